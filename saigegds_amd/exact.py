"""Exact p-values for the ultra-rare rows of a binary-trait scan (``seqAssocGLMM_SPA(exact_mac=)``).

With a handful of carriers the score statistic of a row takes a few dozen values at most, and a continuous
approximation of its tail -- the normal one and the saddlepoint one alike -- can be off by a large factor in either
direction.  SAIGE proper answers with "efficient resampling" (``--max_MAC_for_ER``); the reference has nothing of the
kind, so nothing here mirrors reference code and no reference vector pins it; the definition is DESIGN.md 8l.

For a row with the scan's own dosage table ``t`` (mean imputation and the flip to the minor allele,
``firth.firth_tables``) the carriers are the samples with a hard call of dosage 1 or 2, ``MAC`` their dosage sum.  The
scan's score is ``T = A - m'`` with ``A = sum_carriers g y``, an integer in ``0..MAC``; under the null the carriers'
``y`` are independent Bernoulli(``mu``), which gives ``A`` a weighted Poisson-binomial pmf ``f`` built one carrier at a
time.  Missing genotypes (imputed to ``t[3]``) are not resampled: they shift the centre, ``m' = sum_carriers g mu -
t[3] sum_missing (y - mu)``.  With ``d_a = |a - m'|``,

    pval.exact.full = sum_{d_a >= d_obs} f[a],    pval.exact = sum_{d_a > d_obs} f[a] + 1/2 sum_{d_a == d_obs} f[a]

(the mid-p correction).  The test treats the samples as independent: like SAIGE's efficient resampling it uses
neither the variance ratio nor the GRM.

``exact_pass`` is the host side: it takes the rows in batches of bounded bytes -- their 2-bit rows
(``ScanInput.packed_rows_at``), the tables from the ``AF.alt`` column, and ``Scanner.exact_2bit`` (``sgx_exact_2bit``,
kern_exact.h).  Hard calls only: where ``A`` is no integer (true dosages) the test is not defined.  Out of scope: the
set-test and conditional drivers, more than one GPU.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Tuple

import numpy as np

from . import firth

EXACT_MAX_MAC = 63              # SGX_EXACT_MAX_MAC: f[a] lives in lane a of one wave
NO_DOSAGE = "Exact p-values on dosage input are not implemented: the test needs hard calls."


def exact_input(inp):
    """The opened input of a driver call as the exact pass takes it: 2-bit rows as they are, an in-memory uint8 / int32
    matrix that holds 0, 1, 2 and the missing code only as the rows it means (``aggregate.reduce_hard_calls``).  Any
    other input -- a dosage node, a file of dosages only, a matrix of other values -- is refused."""
    inp = firth.hard_call_input(inp)
    if inp.kind != "packed":
        raise NotImplementedError(NO_DOSAGE)
    return inp


def exact_pass(inp, out: np.ndarray, valid: np.ndarray, rows, make_scanner: Callable,
               max_mac: int) -> Tuple[np.ndarray, np.ndarray]:
    """Exact p-values of the variants ``rows`` (0-based indices into the input's variants) of a finished scan: ``out``
    [n_var, 8] and ``valid`` [n_var] are the scan's table and flags.  ``make_scanner()`` gives an object for the model of
    these rows with ``close()`` and ``exact_2bit(packed, lut, max_mac)``.  -> (p.mid, p.full), each [n_var]: NaN off
    ``rows``, on rows that are not valid and on rows the kernel does not finish (more than ``max_mac`` minor alleles)."""
    n_var = out.shape[0]
    mid, full = np.full(n_var, np.nan), np.full(n_var, np.nan)
    rows = firth.valid_rows(rows, valid)
    if rows.size == 0:
        return mid, full
    if inp.kind != "packed":
        raise NotImplementedError(NO_DOSAGE)
    with contextlib.closing(make_scanner()) as sc:
        for idx, packed, lut, _ in firth.hard_call_batches(inp, out, rows):
            o4 = np.asarray(sc.exact_2bit(packed, lut, int(max_mac)))
            done = o4[:, 3] == 1
            mid[idx[done]], full[idx[done]] = o4[done, 0], o4[done, 1]
    return mid, full


def follow_up(inp, max_mac: int, mac) -> firth.FollowUp:
    """``seqAssocGLMM_SPA(exact_mac=)`` of a scan with the filter ``mac``: the exact pass of every valid row with
    ``mac <= exact_mac``.  True dosages are refused here."""
    inp = exact_input(inp)
    return firth.FollowUp(
        f"    MAC threshold for exact p-values: {max_mac} (rows below the MAC threshold above, {mac}, are "
        "never valid: lower `mac` to reach them)",
        (("pval.exact", np.nan, np.float64), ("pval.exact.full", np.nan, np.float64)),
        lambda out, valid: (valid != 0) & (out[:, 1] <= max_mac),
        lambda out, valid, rows, make_scanner: exact_pass(inp, out, valid, rows, make_scanner, int(max_mac)))
