"""Host driver of the single-variant scan: Python mirror of
``seqAssocGLMM_SPA()`` (reference R/assoc_single.r:92-334) over the C ABI.

Same arguments, same checks and messages, same result columns.  ``parallel``
is reinterpreted as the number of GPUs driven from this process (the reference
forks SeqArray worker processes instead, R/assoc_single.r:167-204).
"""
from __future__ import annotations

import math
import re
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Union

import numpy as np

from .gds import GdsError, GdsFile, pack_dosage_2bit, unpack_dosage_2bit
from .nullmod import ModelError, NullModel, ScanModel, init_nullmod, load_modobj

BLOCK_SIZE = 50_000   # .bl_size=50000L, R/assoc_single.r:204


PACKED_BLOCK_BYTES = 1 << 30   # host bytes of one block of packed-real rows as the file stores them


def packed_block_size(raw_row_bytes: int) -> int:
    """Variants per block on the stored-rows routes (packed-real dosages, genotype/data): .bl_size, but no more than a
    GiB of stored rows -- a block is read and held whole on the host, and at N = 430 000 a 16-bit row is 0.86 MB
    (50 000 of them: 43 GB), a row of allele codes 215 kB (10.75 GB)."""
    return min(BLOCK_SIZE, max(1, PACKED_BLOCK_BYTES // int(raw_row_bytes)))


class PackedRows:
    """Rows of a packed-real (or float32) dosage node as stored (``GdsFile.dosage_raw_range``) with what the device
    needs to decode them: the node's class, scale and offset, and the model's samples as indices into the file's
    (None: the file's samples are the model's, in order).  What ``Scanner.scan_packed`` / ``DosageBlock.load_packed``
    take."""

    def __init__(self, raw: np.ndarray, cls: str, scale: float, offset: float, sel: Optional[np.ndarray]):
        self.raw, self.cls, self.scale, self.offset, self.sel = raw, cls, scale, offset, sel

    @property
    def nbytes(self) -> int:
        return self.raw.nbytes

    def args(self):
        return self.raw, self.cls, self.scale, self.offset, self.sel


# Where the allele codes of genotype/data become 2-bit dosage rows: "device" -- the stored rows cross PCIe as they are
# and sgx_scan_dbit2 decodes and sample-selects them; "host" -- dosage_alt_packed_range (sgx_decode_dbit2 on the host's
# threads), then sgx_scan_2bit.  Same table either way, bit for bit.
GENOTYPE_DECODE = "device"
MAX_STORED_ROWS = 16      # SGX_DBIT2_MAX_ROWS: stored rows of one variant sgx_scan_dbit2 takes; a block with a wider site is decoded on the host


class StoredGenotypes:
    """Rows of genotype/data as stored (``GdsFile.genotype_raw_range``) with what the device needs to decode them: the
    bit the first row starts at, the file's samples per row, the rows per variant (None: one each) and the model's
    samples as indices into the file's (None: the file's samples are the model's, in order).  What
    ``Scanner.scan_dbit2`` / ``Block.load_dbit2`` take."""

    def __init__(self, raw: np.ndarray, bit0: int, n_file_samp: int, n_rows: Optional[np.ndarray], sel: Optional[np.ndarray],
                 n_variants: int):
        self.raw, self.bit0, self.n_file_samp, self.n_rows, self.sel, self.n_variants = raw, bit0, n_file_samp, n_rows, sel, n_variants

    @property
    def nbytes(self) -> int:
        return self.raw.nbytes

    def args(self):
        return self.raw, self.bit0, self.n_file_samp, self.n_rows, self.sel, self.n_variants


class GenotypeSource:
    """In-memory stand-in for an opened SeqArray GDS file (synthetic data,
    tests): 2-bit packed ``$dosage_alt`` rows or real-valued dosages."""

    def __init__(self, sample_id: List[str], packed: Optional[np.ndarray] = None,
                 dosage: Optional[np.ndarray] = None, variant_id=None, chromosome=None,
                 position=None, rs_id=None, ref=None, alt=None):
        if (packed is None) == (dosage is None):
            raise ValueError("give exactly one of packed / dosage")
        self._sample_id = list(sample_id)
        self.packed, self.dosage = packed, dosage
        m = (packed if packed is not None else dosage).shape[0]
        self.variant_id = np.arange(1, m + 1) if variant_id is None else np.asarray(variant_id)
        self.chromosome = ["1"] * m if chromosome is None else list(chromosome)
        self.position = np.arange(1, m + 1) if position is None else np.asarray(position)
        self.rs_id = rs_id
        self.ref = ["A"] * m if ref is None else list(ref)
        self.alt = ["C"] * m if alt is None else list(alt)

    def sample_id(self):
        return self._sample_id


def _open_source(gdsfile, verbose):
    if isinstance(gdsfile, GenotypeSource):
        return gdsfile
    if isinstance(gdsfile, str):
        if verbose:
            print(f"    open '{gdsfile}'")
        gdsfile = GdsFile(gdsfile)
    if not isinstance(gdsfile, GdsFile):
        raise TypeError("inherits(gdsfile, \"SeqVarGDSClass\") | is.character(gdsfile) is not TRUE")
    return gdsfile


def _dsnode(src, nm: str) -> str:
    """``.dsnode`` (R/assoc_single.r:69-85)."""
    if not isinstance(nm, str):
        raise TypeError("is.character(dsnode) is not TRUE")
    if isinstance(src, GenotypeSource):
        return "$dosage_alt" if src.packed is not None else "annotation/format/DS"
    if nm == "":
        if src.node("genotype/data", silent=True) is not None:
            return "$dosage_alt"
        nm = "annotation/format/DS"
        if src.node(nm, silent=True) is None:
            raise GdsError("Dosages should be stored in genotype or annotation/format/DS.")
    return nm


def match_samples(src, mod):
    """The model's samples in the genotype source (R/assoc_single.r:135-142) -> (the source's sample ids, the indices
    ``sel`` (int64) of the model's samples among them in the source's order, ``ii``: their rows in the model)."""
    gsid = [str(s) for s in src.sample_id()]
    pos = {str(s): i for i, s in enumerate(mod.sample_id)}
    sel = [i for i, s in enumerate(gsid) if s in pos]
    if len(sel) != len(mod.sample_id):
        raise ModelError("Some of sample IDs are not available in the GDS file.")
    ii = np.array([pos[gsid[i]] for i in sel], dtype=np.int64)
    return gsid, np.asarray(sel, dtype=np.int64), ii


@dataclass(frozen=True)
class ScanInput:
    """The opened input of one driver call (``open_scan_input``): where the genotypes come from, which of the source's
    samples are the model's, and how rows are read for them.  Nothing is decoded when it is made (the reference never
    holds more than one block of .bl_size variants either, R/assoc_single.r:202-209)."""
    src: Any                    # GenotypeSource or GdsFile
    in_mem: bool                # src is a GenotypeSource
    node: str                   # "$dosage_alt", or the dosage node
    kind: str                   # "packed": 2-bit hard calls; "dosage": rows decoded on the host; "stored": a packed-real
    #                             or float32 node, whose rows can cross PCIe as the file stores them
    n_var: int
    n_all: int                  # samples of the source
    gsid: List[str]             # their ids
    sel: np.ndarray             # int64: the model's samples among them, in the source's order
    ii: np.ndarray              # int64: their rows in the model
    all_samples: bool           # the source's samples are the model's, in order
    packed: Optional[np.ndarray] = None     # in-memory 2-bit rows
    ds_all: Optional[np.ndarray] = None     # in-memory dosage matrix
    ds_dtype: Optional[np.dtype] = None     # dosage input: the type of the decoded rows

    @property
    def n_samp(self) -> int:
        return self.sel.size

    def sample_id(self) -> List[str]:
        return [self.gsid[i] for i in self.sel]

    def _select(self, rows: np.ndarray) -> np.ndarray:
        """2-bit rows of the source's samples -> of the model's."""
        return rows if self.all_samples else pack_dosage_2bit(unpack_dosage_2bit(rows, self.n_all)[:, self.sel])

    def packed_rows(self, off: int, end: int) -> np.ndarray:
        """2-bit rows of variants [off, end) for the model's samples (host decoder)."""
        if self.in_mem:
            return self._select(self.packed[off:end])
        return self.src.dosage_alt_packed_range(off, end, None if self.all_samples else self.sel)

    def packed_rows_at(self, idx: np.ndarray) -> np.ndarray:
        """... of the variants ``idx`` (0-based, ascending); a file is decoded whole, once."""
        return np.ascontiguousarray(self._select((self.packed if self.in_mem else self.src.dosage_alt_packed()[0])[idx]))

    def read_block(self, off: int, end: int):
        """Genotypes of variants [off, end) for the model's samples, as ``scan_blocks`` takes them."""
        sel = None if self.all_samples else self.sel
        if self.kind == "packed":
            if not self.in_mem and GENOTYPE_DECODE == "device":
                raw, bit0, reps = self.src.genotype_raw_range(off, end)
                if reps is None or int(reps.max()) <= MAX_STORED_ROWS:      # (the host decoder has no such limit)
                    return StoredGenotypes(raw, bit0, self.n_all, reps, sel, end - off)
            return self.packed_rows(off, end)
        if self.kind == "stored":
            return PackedRows(*self.src.dosage_raw_range(self.node, off, end), sel)
        blk = self.ds_all[off:end] if self.in_mem else self.src.dosage_real_range(self.node, off, end)
        return blk if self.all_samples else np.ascontiguousarray(blk[:, self.sel])

    def stored_ok(self, scanner_factory) -> bool:
        """A packed-real or float32 node goes to the device as stored: the variants are picked on the host, the
        samples there.  (An injected scanner -- the tests' CPU stand-in for the device -- has no such load: decoded
        rows.)"""
        return self.kind == "stored" and scanner_factory is None

    def dosage_reader(self, stored: bool):
        """``read_rows(v0)`` of the dosage drivers: 0-based variant indices, ascending -> their rows for the model's
        samples.  ``stored`` (``stored_ok``): ``PackedRows`` [len, n_all] of the file's samples, the model's picked
        on the device; else decoded rows [len, n_samp] of ``ds_dtype``."""
        src, node = self.src, self.node

        def read_stored(v0):
            step = packed_block_size(src.dosage_raw_row_bytes(node))
            parts, meta = [], None
            for a in range(int(v0[0]), int(v0[-1]) + 1, step):          # the range in pieces of a bounded size
                pick = v0[(v0 >= a) & (v0 < a + step)]
                if pick.size:
                    raw, *meta = src.dosage_raw_range(node, int(pick[0]), int(pick[-1]) + 1)
                    parts.append(raw[pick - pick[0]])
            return PackedRows(np.concatenate(parts), *meta, None if self.all_samples else self.sel)

        def read_rows(v0):
            if self.in_mem:
                rows = self.ds_all[v0]
            else:
                lo = int(v0[0])
                rows = src.dosage_real_range(node, lo, int(v0[-1]) + 1)[v0 - lo]
            return np.ascontiguousarray(rows if self.all_samples else rows[:, self.sel], dtype=self.ds_dtype)
        return read_stored if stored else read_rows


def open_scan_input(gdsfile, mod, dsnode: str, verbose: bool, any_matrix: bool = False) -> ScanInput:
    """Open the genotype source of a driver call, match the model's samples in it and classify it.  An in-memory
    dosage matrix is [variant, sample] of uint8, int32 or float64, unless ``any_matrix`` (the single-variant driver:
    its scanner converts what it is given)."""
    src = _open_source(gdsfile, verbose)
    gsid, sel, ii = match_samples(src, mod)
    node = _dsnode(src, dsnode)
    in_mem, n_all = isinstance(src, GenotypeSource), len(gsid)
    packed = ds_all = ds_dtype = None
    if in_mem and src.packed is not None:
        kind, packed, n_var = "packed", src.packed, src.packed.shape[0]
    elif in_mem:
        ds_all = src.dosage if any_matrix else np.asarray(src.dosage)
        if not any_matrix and (ds_all.ndim != 2 or ds_all.shape[1] != n_all or ds_all.dtype not in (np.uint8, np.int32, np.float64)):
            raise TypeError("the dosages should be a [variant, sample] matrix of uint8, int32 or float64")
        kind, n_var, ds_dtype = "dosage", ds_all.shape[0], ds_all.dtype
    elif node == "$dosage_alt":
        kind = "packed"
        n_var, n_all = src.genotype_dims()
    else:
        kind = "dosage" if src.dosage_raw_class(node) is None else "stored"
        n_var, n_all = src.node(node + "/data").dims[:2]
        ds_dtype = np.dtype(np.float64)
    all_samples = sel.size == n_all and np.array_equal(sel, np.arange(n_all))
    return ScanInput(src, in_mem, node, kind, n_var, n_all, gsid, sel, ii, all_samples, packed, ds_all, ds_dtype)


def _pretty(n: int) -> str:
    return f"{n:,}"


def _is_num(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def check_scan_args(maf, mac, missing, spa_pval, var_ratio, dsnode, res_savefn, res_compress, verbose=True):
    """The argument checks of R/assoc_single.r:96-107, in its order."""
    for nm, v in (("maf", maf), ("mac", mac), ("missing", missing), ("spa.pval", spa_pval), ("var.ratio", var_ratio)):
        if not _is_num(v):
            raise TypeError(f"is.numeric({nm}) is not TRUE")
    if not isinstance(dsnode, str):
        raise TypeError("is.character(dsnode) is not TRUE")
    if not isinstance(res_savefn, str):
        raise TypeError("is.character(res.savefn) is not TRUE")
    if res_compress not in ("LZMA", "LZMA_RA", "ZIP", "ZIP_RA", "none"):
        raise ValueError("`res.compress` should be one of LZMA, LZMA_RA, ZIP, ZIP_RA and none.")
    if not isinstance(verbose, bool):
        raise TypeError("is.logical(verbose) is not TRUE")


def require_device(what: str) -> int:
    """The number of visible devices; none is an error (there is no CPU path)."""
    from ._lib import load
    ndev = load().sgx_device_count()
    if ndev <= 0:
        raise RuntimeError(f"{what}: no MI355X device is visible (there is no CPU fallback)")
    return ndev


def finish_result(ans, res_savefn: str, res_compress: str, verbose: bool, sample_id):
    """The tail of a scan driver (R/assoc_single.r:236-334): the table, or None once it is saved to ``res_savefn``."""
    if res_savefn:
        from .results import save_result
        if verbose:
            print(f"Save to '{res_savefn}' ...")
        save_result(ans, res_savefn, res_compress, sample_id=sample_id)
        ans = None
    if verbose:
        print("Done.")
    return ans


def seqAssocGLMM_SPA(gdsfile: Union[str, GdsFile, GenotypeSource], modobj: Any, maf: float = float("nan"),
                     mac: float = 10, missing: float = 0.1, dsnode: str = "", spa_pval: float = 0.05,
                     var_ratio: float = float("nan"), res_savefn: str = "", res_compress: str = "LZMA",
                     parallel: Union[bool, int] = False, verbose: bool = True, timing: Optional[Dict[str, float]] = None,
                     firth_pval: Optional[float] = None, firth_maxit: int = 50, exact_mac: Optional[int] = None):
    """SAIGE single-variant association scan on MI355X.

    Returns a ``dict`` of equal-length columns (``pandas.DataFrame(result)``
    gives the reference's data.frame): id, chr, pos, [rs.id], ref, alt, AF.alt,
    mac, num, beta, SE, pval and, for binary traits, p.norm, converged
    (man/seqAssocGLMM_SPA.Rd:60-74).

    ``firth_pval`` (not in the reference; binary traits; every input the scan takes: hard calls by ``sgx_firth_2bit``,
    dosages by ``sgx_ds_block_firth`` on a resident dosage block): a number in (0, 1] -- after the scan every valid row with ``pval <= firth_pval`` gets a Firth bias-reduced fit (``saigegds_amd.firth``; at most
    ``firth_maxit`` iterations) on device 0, with a LOCO model against its chromosome's model, and the result gains
    ``beta.firth`` (for the alt allele, like ``beta``), ``SE.firth`` and ``cvg.firth`` (NaN / NaN / False on the other
    rows).  None: no such columns and no such pass.  ``res_savefn``: ``.rds`` / ``.RData``; the ``.gds`` writer has
    fixed columns and is refused.

    ``exact_mac`` (not in the reference; SAIGE proper's ``--max_MAC_for_ER``; binary traits; hard calls only): an
    integer in 1..63 -- after the scan every valid row with ``mac <= exact_mac`` gets the exact null distribution of
    its score over the carriers' phenotypes (``saigegds_amd.exact``; ``sgx_exact_2bit``) on device 0, with
    a LOCO model against its chromosome's model, and the result gains ``pval.exact`` (mid-p) and ``pval.exact.full``
    (NaN on the other rows).  The test takes the samples as independent: neither the variance ratio nor the GRM
    enters.  Rows below the scan's own ``mac`` filter (default 10) are never valid: lower ``mac`` for the option to
    bite.  None: no such columns and no such pass.  It combines freely with ``firth_pval``; the ``.gds`` writer is
    refused as for it.
    """
    check_scan_args(maf, mac, missing, spa_pval, var_ratio, dsnode, res_savefn, res_compress, verbose)
    if firth_pval is not None:
        if not _is_num(firth_pval) or not 0 < firth_pval <= 1:
            raise ValueError("`firth_pval` should be None or a number in (0, 1].")
        if not isinstance(firth_maxit, (int, np.integer)) or isinstance(firth_maxit, bool) or firth_maxit < 1:
            raise ValueError("`firth_maxit` should be a positive integer.")
        if re.search(r"\.gds$", res_savefn, re.I):
            raise ValueError("The gds output has no columns for the Firth effect sizes; save to RData or RDS.")
    if exact_mac is not None:
        if not isinstance(exact_mac, (int, np.integer)) or isinstance(exact_mac, bool) or not 1 <= exact_mac <= 63:
            raise ValueError("`exact_mac` should be None or an integer in 1..63.")
        if re.search(r"\.gds$", res_savefn, re.I):
            raise ValueError("The gds output has no columns for the exact p-values; save to RData or RDS.")
    if verbose:
        print("SAIGE association analysis:")

    if GENOTYPE_DECODE not in ("device", "host"):
        raise ValueError("saigegds_amd.assoc.GENOTYPE_DECODE should be 'device' or 'host'.")
    mod: NullModel = load_modobj(modobj, verbose)
    src = _open_source(gdsfile, verbose)
    _dsnode(src, dsnode)      # (a file without dosages is refused before its samples are looked at, R/assoc_single.r:133)
    inp = open_scan_input(src, mod, dsnode, verbose, any_matrix=True)
    kind, n_samp, n_var, ii = inp.kind, inp.n_samp, inp.n_var, inp.ii
    passes = []               # the per-row follow-ups (firth.FollowUp), in the order of their columns
    if firth_pval is not None:
        from . import _lib, firth
        if mod.trait_type != "binary":
            raise ValueError("Firth effect sizes are for binary traits.")
        passes.append(firth.follow_up(inp, _lib.Scanner, firth_pval, firth_maxit))      # (no dosage route: NotImplementedError)
    if exact_mac is not None:
        from . import exact
        if mod.trait_type != "binary":
            raise ValueError("Exact p-values are for binary traits.")
        passes.append(exact.follow_up(inp, int(exact_mac), mac))                         # (true dosages: NotImplementedError)
    if verbose:
        print(f"    # of samples: {_pretty(n_samp)}")
        print(f"    # of variants: {_pretty(n_var)}")
        print(f"    MAF threshold: {maf}")
        print(f"    MAC threshold: {mac}")
        print(f"    missing threshold for variants: {missing}")
        print(f"    p-value threshold for SPA adjustment: {spa_pval}")
        for p in passes:
            print(p.note)
    if not math.isfinite(var_ratio):
        var_ratio = float(np.nanmean(mod.var_ratio))
    if verbose:
        print(f"    variance ratio for approximation: {var_ratio}")
    if n_samp <= 0:
        raise ValueError("No sample in the genotypic data set!")
    if n_var <= 0:
        raise ValueError("No variant in the genotypic data set!")

    mobj: ScanModel = init_nullmod(mod, ii, maf, mac, missing, spa_pval, var_ratio)
    if mod.trait_type not in ("binary", "quantitative"):
        raise ModelError("Invalid 'modobj$trait.type'.")

    # devices, R/assoc_single.r:167-171 ('parallel' = number of GPUs here)
    from ._lib import Scanner
    ngpu = 1 if parallel in (False, None, 0, 1) else int(parallel)
    ndev = require_device("seqAssocGLMM_SPA")
    if ngpu > ndev:
        raise ValueError(f"parallel={ngpu} but only {ndev} GPU(s) are visible")
    if verbose:
        print(f"    # of GPUs: {ngpu}")

    # scan by blocks of .bl_size variants, R/assoc_single.r:199-223; results land at the blocks' own
    # offsets, so the table keeps the file's order whatever GPU finishes first (:226-227)
    out = np.empty((n_var, 8), dtype=np.float64)
    valid = np.zeros(n_var, dtype=np.uint8)
    bl_size = BLOCK_SIZE
    if kind == "stored":
        bl_size = packed_block_size(src.dosage_raw_row_bytes(inp.node))
    elif kind == "packed" and not inp.in_mem and GENOTYPE_DECODE == "device":
        bl_size = packed_block_size(src.genotype_raw_row_bytes())      # a stored row is twice a 2-bit row
    t_loop = time.perf_counter()
    cols = {name: np.full(n_var, fill, dtype=dt) for p in passes for name, fill, dt in p.columns}
    for p in passes:
        p.ready(lambda: Scanner(mobj, device=0))

    def follow_ups(r0, r1, obj):
        """Every follow-up pass of the scanned rows [r0, r1) against the model they were scanned with."""
        for p in passes:
            with np.errstate(invalid="ignore"):
                rows = r0 + np.flatnonzero(p.flagged(out[r0:r1], valid[r0:r1]))
            for (name, _, _), g in zip(p.columns, p.run(out, valid, rows, lambda: Scanner(obj, device=0))):
                cols[name][rows] = g[rows]

    if not mod.loco:
        blocks = [(off, min(n_var, off + bl_size)) for off in range(0, n_var, bl_size)]
        scan_blocks(lambda d: Scanner(mobj, device=d), ngpu, blocks, inp.read_block, kind == "packed", out, valid, timing)
        follow_ups(0, n_var, mobj)
    else:
        # leave-one-chromosome-out: the block list is cut at chromosome boundaries, and every run of one
        # chromosome is scanned against that chromosome's model (its fitted values; y, V, XV, XXVX_inv and
        # the variance ratio are the full model's) by scanners of its own, freed before the next run
        chrom = [str(c) for c in (src.chromosome if inp.in_mem else src.read("chromosome"))]
        reported = set()
        for r0, r1, ch in chromosome_runs(chrom):
            if ch in mod.loco:
                run_obj = init_nullmod(mod.for_chromosome(ch), ii, maf, mac, missing, spa_pval, var_ratio)
            else:
                run_obj = mobj
                if verbose and ch not in reported:
                    print(f"    chromosome '{ch}' has no leave-one-chromosome-out model: the full model is used")
                reported.add(ch)
            blocks = [(off, min(r1, off + bl_size)) for off in range(r0, r1, bl_size)]
            scan_blocks(lambda d, o=run_obj: Scanner(o, device=d), ngpu, blocks, inp.read_block, kind == "packed", out, valid,
                        timing)
            follow_ups(r0, r1, run_obj)
    if timing is not None:
        timing["blocks_s"] = time.perf_counter() - t_loop      # handles + every block (decode and scan overlapped)

    x = valid.astype(bool)           # R/assoc_single.r:225-234
    if verbose:
        print("# of variants after filtering by MAF, MAC and missing thresholds: "
              f"{_pretty(int(x.sum()))}")
    ans = assemble_result(src, x, out, mod.trait_type)
    ans.update((name, c[x]) for name, c in cols.items())
    return finish_result(ans, res_savefn, res_compress, verbose, inp.sample_id() if res_savefn else None)


def chromosome_runs(chrom):
    """Maximal runs of equal consecutive values -> [(start, end, value)]."""
    runs = []
    for i, c in enumerate(chrom):
        if runs and runs[-1][2] == c:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1, c])
    return [tuple(r) for r in runs]


def scan_blocks(make_scanner, ngpu: int, blocks, read_block, packed_rows: bool, out: np.ndarray, valid: np.ndarray,
                timing: Optional[Dict[str, float]] = None):
    """One host thread per GPU (the reference forks one SeqArray worker per core, seqParallel,
    R/assoc_single.r:202-204): each thread owns a scanner and pulls blocks from a shared queue.  Every
    scanner has a decoder thread of its own one block ahead of it: while block i crosses PCIe and is
    scanned (the C ABI call releases the GIL), block i + 1 is being read and decoded (lzma / zlib and
    numpy release the GIL), so neither the GPU nor the decoder waits for the other beyond the slower of
    the two.  timing: seconds spent decoding / scanning (summed over threads) and decoded bytes."""
    import queue
    import threading
    import time
    from concurrent.futures import ThreadPoolExecutor
    todo: "queue.Queue" = queue.Queue()
    for b in blocks:
        todo.put(b)
    errors: List[BaseException] = []
    tlock = threading.Lock()

    def take():
        try:
            return todo.get_nowait()
        except queue.Empty:
            return None

    def decode(rng):
        t = time.perf_counter()
        blk = read_block(*rng)
        if timing is not None:
            with tlock:
                timing["decode_s"] = timing.get("decode_s", 0.0) + time.perf_counter() - t
                timing["decoded_bytes"] = timing.get("decoded_bytes", 0.0) + blk.nbytes
        return blk

    def worker(d: int):
        sc = None
        try:
            sc = make_scanner(d)
            with ThreadPoolExecutor(1, thread_name_prefix=f"sgx-decode{d}") as ex:
                rng = take()
                fut = ex.submit(decode, rng) if rng is not None else None
                while fut is not None and not errors:
                    off, end = rng
                    blk = fut.result()
                    rng = take()                                       # the next block decodes while this one is scanned
                    fut = ex.submit(decode, rng) if rng is not None else None
                    t = time.perf_counter()
                    if isinstance(blk, StoredGenotypes):
                        o, v = sc.scan_dbit2(*blk.args())   # genotype/data rows as stored: decoded on the device
                    elif packed_rows:
                        o, v = sc.scan_2bit(blk)            # 2-bit packed rows
                    elif isinstance(blk, PackedRows):
                        o, v = sc.scan_packed(*blk.args())  # packed-real rows as stored: decoded on the device
                    elif blk.dtype == np.uint8:
                        o, v = sc.scan_u8(blk)
                    elif np.issubdtype(blk.dtype, np.integer):
                        o, v = sc.scan_i32(blk)
                    else:
                        o, v = sc.scan_f64(blk)
                    out[off:end], valid[off:end] = o, v
                    if timing is not None:
                        with tlock:
                            timing["scan_s"] = timing.get("scan_s", 0.0) + time.perf_counter() - t
        except BaseException as e:      # noqa: BLE001 -- re-raised in the caller's thread
            errors.append(e)
        finally:
            if sc is not None:
                sc.close()

    if ngpu == 1:
        worker(0)
    else:
        threads = [threading.Thread(target=worker, args=(d,), name=f"sgx-gpu{d}") for d in range(ngpu)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]


def assemble_result(src, keep: np.ndarray, out: np.ndarray, trait_type: str) -> Dict[str, Any]:
    """The data.frame of R/assoc_single.r:287-308 as an ordered dict of columns."""
    def sub(a):
        return [v for v, k in zip(a, keep) if k] if isinstance(a, list) else np.asarray(a)[keep]
    if isinstance(src, GenotypeSource):
        vid, chrom, posn, rs = src.variant_id, src.chromosome, src.position, src.rs_id
        ref, alt = src.ref, src.alt
    else:
        vid, chrom, posn = src.read("variant.id"), src.read("chromosome"), src.read("position")
        rs = src.read("annotation/id") if src.node("annotation/id", silent=True) is not None else None
        ref, alt = src.alleles()
    o = out[keep]
    ans: Dict[str, Any] = {"id": sub(vid), "chr": sub(list(chrom)), "pos": sub(posn)}
    if rs is not None:
        ans["rs.id"] = sub(list(rs))
    ans["ref"], ans["alt"] = sub(list(ref)), sub(list(alt))
    ans["AF.alt"], ans["mac"] = o[:, 0].copy(), o[:, 1].copy()
    ans["num"] = o[:, 2].astype(np.int32)
    ans["beta"], ans["SE"], ans["pval"] = o[:, 3].copy(), o[:, 4].copy(), o[:, 5].copy()
    if trait_type == "binary":
        ans["p.norm"] = o[:, 6].copy()
        ans["converged"] = o[:, 7] == 1
    return ans
