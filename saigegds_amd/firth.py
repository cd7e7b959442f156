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

``firth_pass`` is the host side: it takes the flagged rows in batches of bounded bytes.  Hard calls (``genotype/data``,
packed in-memory rows, an in-memory uint8 / int32 matrix of hard calls): their 2-bit rows (``ScanInput.packed_rows_at``:
in-memory sources, host-decoded and device-decoded files alike), the tables from the ``AF.alt`` column, and
``Scanner.firth_2bit`` (``sgx_firth_2bit``, kern_firth.h).  Dosages (a ``dsnode``, a file of ``annotation/format/DS``
alone, a stored packed-real or float32 node, any other in-memory matrix): the rows by ``ScanInput.dosage_reader`` -- a
stored node in its file form -- into one resident ``DosageBlock``, flip and mean from the load's own counts
(``aggregate.flip_mean``, as the conditional driver), and ``DosageBlock.firth`` (``sgx_ds_block_firth``,
kern_firth_ds.h).  Dosage input on a scanner without ``dosage_block``, or whose block has no ``firth``, is refused.
Out of scope: the set-test and conditional drivers, more than one GPU.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Callable, NamedTuple, Tuple

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


class FollowUp(NamedTuple):
    """One per-row follow-up of ``seqAssocGLMM_SPA``, as the driver runs it after each ``scan_blocks`` call."""
    note: str                   # the verbose line of the option
    columns: tuple              # ((name, fill value, dtype), ...) of the result
    flagged: Callable           # (out, valid) of scanned rows -> their mask
    run: Callable               # (out, valid, rows, make_scanner) -> the column arrays [n_var], read at rows
    ready: Callable = lambda make_scanner: None      # what is refused before any row is scanned


def hard_call_input(inp):
    """An in-memory uint8 / int32 matrix of hard calls as 2-bit rows (``aggregate.reduce_hard_calls``), else ``inp``."""
    if inp.kind == "dosage" and inp.in_mem:
        ds = np.asarray(inp.ds_all)
        if ds.ndim == 2 and ds.dtype in (np.uint8, np.int32):
            inp = aggregate.reduce_hard_calls(dataclasses.replace(inp, ds_all=ds, ds_dtype=ds.dtype))
    return inp


def valid_rows(rows, valid) -> np.ndarray:
    """Row indices as a pass takes them: unique and ascending, the valid ones."""
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    return rows[np.asarray(valid)[rows] != 0]


def hard_call_batches(inp, out: np.ndarray, rows: np.ndarray):
    """Batches of ``FIRTH_BATCH_BYTES`` of the 2-bit rows ``rows`` -> (idx, packed rows, tables from ``AF.alt``, flip)."""
    per = max(1, FIRTH_BATCH_BYTES // max(1, (inp.n_samp + 3) // 4))
    for a in range(0, rows.size, per):
        idx = rows[a:a + per]
        lut, flip = firth_tables(out[idx, 0])
        yield idx, inp.packed_rows_at(idx), lut, flip


def firth_input(inp, scanner_cls):
    """The opened input of a driver call as the Firth pass takes it: hard calls as 2-bit rows -- as they are, or an
    in-memory uint8 / int32 matrix that holds 0, 1, 2 and the missing code only as the rows it means
    (``aggregate.reduce_hard_calls``); any other input -- a dosage node, a file of dosages only, a matrix of other
    values -- as dosage rows of the type the scan gives them (uint8, int32 for other integers, else float64), refused
    where ``scanner_cls`` has no ``dosage_block``."""
    inp = hard_call_input(inp)
    if inp.kind == "packed":
        return inp
    if not hasattr(scanner_cls, "dosage_block"):
        raise NotImplementedError(NO_DOSAGE)
    if inp.in_mem:
        ds = np.asarray(inp.ds_all)
        dt = ds.dtype if ds.dtype == np.uint8 else np.dtype(np.int32 if np.issubdtype(ds.dtype, np.integer) else np.float64)
        inp = dataclasses.replace(inp, ds_all=ds, ds_dtype=dt)
    return inp


def dosage_route(inp, make_scanner) -> bool:
    """Dosage input, before any row is scanned: the scanner's dosage block must have ``firth`` (else
    ``NotImplementedError``) -> whether a stored node goes to it in its file form (the block has ``load_packed``)."""
    with contextlib.closing(make_scanner()) as sc, sc.dosage_block(inp.ds_dtype, 1) as blk:
        if not hasattr(blk, "firth"):
            raise NotImplementedError(NO_DOSAGE)
        return inp.kind == "stored" and hasattr(blk, "load_packed")


def firth_pass(inp, out: np.ndarray, valid: np.ndarray, rows, make_scanner: Callable, maxit: int = 50, stored: bool = False):
    """Firth fits of the variants ``rows`` (0-based indices into the input's variants) of a finished scan: ``out``
    [n_var, 8] and ``valid`` [n_var] are the scan's table and flags.  ``make_scanner()`` gives an object for the model of
    these rows with ``close()`` and, for 2-bit input, ``firth_2bit(packed, lut, maxit)``; for dosage input
    ``dosage_block(dtype, max_variants)`` whose block has ``load`` (``stored``, from ``dosage_route``: ``load_packed``)
    and ``firth(var_idx, flip, mean, maxit)``.  -> (beta, SE, converged), each [n_var]: NaN / NaN / False off ``rows``;
    beta refers to the alt allele."""
    n_var = out.shape[0]
    beta, se = np.full(n_var, np.nan), np.full(n_var, np.nan)
    cvg = np.zeros(n_var, dtype=bool)
    rows = valid_rows(rows, valid)
    if rows.size == 0:
        return beta, se, cvg

    def put(idx, flip, o4):
        beta[idx] = np.where(flip, -o4[:, 0], o4[:, 0])
        se[idx] = o4[:, 1]
        cvg[idx] = o4[:, 3] == 1

    with contextlib.closing(make_scanner()) as sc:
        if inp.kind == "packed":
            for idx, packed, lut, flip in hard_call_batches(inp, out, rows):
                put(idx, flip, np.asarray(sc.firth_2bit(packed, lut, int(maxit))))
        else:
            make = getattr(sc, "dosage_block", None)
            if make is None:
                raise NotImplementedError(NO_DOSAGE)
            read_rows, dtype = inp.dosage_reader(stored), inp.ds_dtype
            per = max(1, aggregate.DS_BUDGET // max(1, aggregate.ds_row_bytes(dtype, inp.n_samp)))
            with make(dtype, min(per, rows.size)) as blk:
                if not hasattr(blk, "firth"):
                    raise NotImplementedError(NO_DOSAGE)
                for a in range(0, rows.size, per):
                    idx = rows[a:a + per]
                    n, s, _ = aggregate.load_rows(blk, read_rows(idx))        # the one upload; the load's own counts
                    flip, mean = aggregate.flip_mean(n, s)
                    o4 = np.asarray(blk.firth(np.arange(idx.size, dtype=np.int32), flip, mean, int(maxit)))
                    put(idx, flip != 0, o4)
    return beta, se, cvg


def follow_up(inp, scanner_cls, pval: float, maxit: int) -> FollowUp:
    """``seqAssocGLMM_SPA(firth_pval=, firth_maxit=)``: the Firth pass of every valid row with ``pval <= firth_pval``.
    Input that ``scanner_cls`` cannot serve is refused here, a dosage block without ``firth`` by ``ready``."""
    inp, stored = firth_input(inp, scanner_cls), []           # stored: what ready appends, dosage_route's answer
    return FollowUp(
        f"    p-value threshold for Firth effect sizes: {pval}",
        (("beta.firth", np.nan, np.float64), ("SE.firth", np.nan, np.float64), ("cvg.firth", False, bool)),
        lambda out, valid: (valid != 0) & (out[:, 5] <= pval),
        lambda out, valid, rows, make_scanner: firth_pass(inp, out, valid, rows, make_scanner, maxit, stored[0]),
        lambda make_scanner: stored.append(inp.kind != "packed" and dosage_route(inp, make_scanner)))
