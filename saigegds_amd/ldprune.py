"""seqFitLDpruning -- LD pruning of the GRM markers, the first step of the vignette (upstream SAIGEgds 2.x; the
reference v1.12.5 sends the user to SNPRelate's snpgdsLDpruning for it).  The statistic, the greedy rule and the
blocked form: DESIGN.md 8n.  The pair decisions come from the device LD kernel (``_lib.LdEngine``); this file is the
host walk over them.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import numpy as np

from .assoc import GenotypeSource, _open_source, chromosome_runs
from .gds import pack_dosage_2bit, unpack_dosage_2bit

_PASS_BYTES = 64 << 20        # 2-bit rows read, counted and filtered per pass
_AUTOSOME = re.compile(r"^(?:chr)?([0-9]+)$", re.I)


def _is_autosome(name: str) -> bool:
    m = _AUTOSOME.match(str(name))
    return bool(m) and 1 <= int(m.group(1)) <= 22


class _Rows:
    """The 2-bit rows of the selected samples of a source with hard calls, by ranges of variants."""

    def __init__(self, src, sel: np.ndarray, n_all: int):
        self.src, self.n_all, self.n = src, n_all, int(sel.size)
        self.sel = None if (self.n == n_all and np.array_equal(sel, np.arange(n_all))) else sel
        self.nb = (self.n + 3) // 4

    def read(self, v0: int, v1: int) -> np.ndarray:
        if not isinstance(self.src, GenotypeSource):
            return np.ascontiguousarray(self.src.dosage_alt_packed_range(v0, v1, sample_sel=self.sel)[:, :self.nb])
        blk = np.asarray(self.src.packed)[v0:v1]
        if self.sel is None:
            return np.ascontiguousarray(blk[:, :self.nb])
        return pack_dosage_2bit(unpack_dosage_2bit(blk, self.n_all)[:, self.sel])


def _counts(rows: np.ndarray, n_samp: int, on_gpu: bool):
    """Per row (n_valid, allele_sum) as int64: the device counts, or their numpy statement under an injected engine."""
    if on_gpu:
        from ._lib import geno_stats_2bit
        nv, ac = geno_stats_2bit(rows, n_samp)
        return nv.astype(np.int64), ac.astype(np.int64)
    codes = unpack_dosage_2bit(rows, n_samp)
    valid = codes != 3
    return valid.sum(axis=1).astype(np.int64), np.where(valid, codes, 0).sum(axis=1, dtype=np.int64)


class _Run:
    """The greedy walk over one chromosome run: candidates arrive in file order, a block goes to the engine once the
    position of the candidate after it is known (that decides which window rows retire with the block's push)."""

    def __init__(self, engine, t2: float, bp: int, max_n: Optional[int], block: int):
        self.eng, self.t2, self.bp, self.max_n, self.block = engine, t2, bp, max_n, block
        self.wpos = np.zeros(0, dtype=np.int64)        # positions of the window rows, oldest first
        self.rows: List[np.ndarray] = []
        self.pos: List[int] = []
        self.ids: List = []
        self.kept: List = []
        self.pending = None                            # (kept indices of the last block, their positions)

    def add(self, rows: np.ndarray, pos: np.ndarray, ids: np.ndarray):
        for k in range(rows.shape[0]):
            if len(self.pos) == self.block:
                self._flush()
            self.rows.append(rows[k])
            self.pos.append(int(pos[k]))
            self.ids.append(ids[k])

    def finish(self) -> list:
        if self.pos:
            self._flush()
        self.eng.reset()
        return self.kept

    def _push(self, next_pos: int):
        """The last block's kept rows join the window; what is out of range for ``next_pos`` retires."""
        idx, kpos = self.pending
        self.pending = None
        W = self.wpos.size
        allpos = np.concatenate([self.wpos, kpos])
        n_drop = int(np.searchsorted(allpos, next_pos - self.bp, side="left"))
        if self.max_n is not None:
            n_drop = max(n_drop, allpos.size - self.max_n)
        drop_old, skip_new = min(n_drop, W), max(0, n_drop - W)
        try:
            self.eng.push(idx[skip_new:], drop_old)
        except MemoryError as e:
            raise MemoryError(f"seqFitLDpruning: the window of kept variants ({allpos.size - n_drop:,} rows) does not fit "
                              f"the engine's memory budget; bound it with slide_max_n (or a smaller slide_max_bp).  {e}") from e
        self.wpos = allpos[n_drop:]

    def _flush(self):
        if self.pending is not None:
            self._push(self.pos[0])
        rows, pos = np.stack(self.rows), np.asarray(self.pos, dtype=np.int64)
        mb, W = pos.size, self.wpos.size
        flags = np.asarray(self.eng.block(rows, self.t2))
        if flags.shape != (mb, W + mb):
            raise RuntimeError(f"seqFitLDpruning: the engine returned flags {flags.shape}, expected {(mb, W + mb)}")
        # the kept variants so far, oldest first: their flag columns and positions
        cols = np.concatenate([np.arange(W), np.zeros(mb, dtype=np.int64)])
        kpos = np.concatenate([self.wpos, np.zeros(mb, dtype=np.int64)])
        nk = W
        idx = []
        for i in range(mb):
            lo = int(np.searchsorted(kpos[:nk], pos[i] - self.bp, side="left"))
            if self.max_n is not None:
                lo = max(lo, nk - self.max_n)
            if not flags[i, cols[lo:nk]].any():
                cols[nk], kpos[nk] = W + i, pos[i]
                nk += 1
                idx.append(i)
                self.kept.append(self.ids[i])
        self.pending = (np.asarray(idx, dtype=np.int32), pos[idx])
        self.rows, self.pos, self.ids = [], [], []


def seqFitLDpruning(gdsfile, sample_id: Optional[Sequence[str]] = None, variant_id=None, ld_threshold: float = 0.2,
                    maf: float = 0.005, missing_rate: float = 0.01, slide_max_bp: int = 500_000,
                    slide_max_n: Optional[int] = None, autosome_only: bool = True, save_gdsfn: str = "",
                    verbose: bool = True, engine_factory=None, block: int = 256) -> Dict[str, np.ndarray]:
    """LD-prune the variants of a genotype file -> {chromosome: kept variant ids}, the ``variant_id=`` of
    seqFitNullGLMM_SPA, seqFitSparseGRM and seqFitDenseGRM (``np.concatenate(list(ids.values()))``).

    ``gdsfile``: a path, GdsFile or GenotypeSource with hard calls (a source with dosages only raises
    NotImplementedError); it is read by blocks of rows, never whole.  ``sample_id`` / ``variant_id`` restrict the
    samples and the candidates.  A candidate passes the fit's own marker filter (``maf``, ``missing_rate`` on the
    selected samples; monomorphic rows never pass) and, with ``autosome_only``, lies on chromosome 1..22 (an optional
    leading ``chr``).

    The rule, per run of one chromosome name in file order (positions must not decrease within a run): candidates are
    taken in file order, starting from the first and walking forward; candidate i is kept iff it is not in LD with
    any kept variant k of the run with pos_i - pos_k <= ``slide_max_bp`` -- only the last ``slide_max_n`` kept ones if
    that is given.  In LD at t = ``ld_threshold``: r^2 > t^2 on the samples called in both rows, strictly (DESIGN.md
    8n).  SNPRelate's random start and backward walk are not offered: the result is a function of the file alone, and
    it does not depend on ``block`` (candidates per engine call, at most 256).

    ``engine_factory(n_samp, bytes_per_variant)``: the object that answers ``block`` / ``push`` / ``reset`` /
    ``window_len`` (default: ``_lib.LdEngine``, the device kernel).  A window of kept rows over the engine's memory
    budget raises MemoryError: bound it with ``slide_max_n``.  A non-empty ``save_gdsfn`` writes the kept variants as a
    SeqArray genotype file (the vignette's seqExport step); the export, unlike the pruning pass, holds all kept rows in
    host memory at once (kept variants x ceil(n_samp / 4) bytes: the size of the GRM file the fit then loads whole).
    ``sample_id`` or ``variant_id`` entries that the file does not hold raise ValueError."""
    from .fitnull import _marker_filter
    for name, v, lo, hi in (("ld_threshold", ld_threshold, 0.0, 1.0), ("maf", maf, 0.0, 0.5),
                            ("missing_rate", missing_rate, 0.0, 1.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (lo <= v <= hi):
            raise ValueError(f"'{name}' should be a number in [{lo:g}, {hi:g}].")
    if isinstance(slide_max_bp, bool) or not isinstance(slide_max_bp, (int, np.integer)) or slide_max_bp < 0:
        raise ValueError("'slide_max_bp' should be a non-negative integer.")
    if slide_max_n is not None and (isinstance(slide_max_n, bool) or not isinstance(slide_max_n, (int, np.integer))
                                    or slide_max_n < 1):
        raise ValueError("'slide_max_n' should be None or a positive integer.")
    from ._lib import LD_BLOCK
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not 1 <= block <= LD_BLOCK:
        raise ValueError(f"'block' should be an integer in [1, {LD_BLOCK}].")
    t2 = float(ld_threshold) * float(ld_threshold)

    src = _open_source(gdsfile, verbose)
    is_mem = isinstance(src, GenotypeSource)
    if (src.packed is None) if is_mem else (not src.has_genotype()):
        raise NotImplementedError("seqFitLDpruning needs hard calls ('genotype'); dosage-only input is not supported yet.")
    gsid = [str(s) for s in src.sample_id()]
    if sample_id is None:
        sel = np.arange(len(gsid), dtype=np.int64)
    else:
        want_s, have = set(str(s) for s in sample_id), set(gsid)
        miss = [s for s in want_s if s not in have]
        if miss:
            raise ValueError(f"'sample_id' not in the GDS file: {sorted(miss)[:5]}")
        sel = np.array([i for i, s in enumerate(gsid) if s in want_s], dtype=np.int64)      # (the file's order)
    if sel.size == 0:
        raise ValueError("No sample selected.")
    n_samp = int(sel.size)
    reader = _Rows(src, sel, len(gsid))
    nb = reader.nb

    var_ids = np.asarray(src.variant_id if is_mem else src.read("variant.id"))
    chrom = [str(c) for c in (src.chromosome if is_mem else src.read("chromosome"))]
    position = np.asarray(src.position if is_mem else src.read("position")).astype(np.int64)
    M = var_ids.size
    cand = np.ones(M, dtype=bool)
    if variant_id is not None:
        want_v = np.unique(np.asarray(list(variant_id)))
        miss_v = want_v[~np.isin(want_v, var_ids)]
        if miss_v.size:
            raise ValueError(f"'variant_id' not in the GDS file: {miss_v[:5].tolist()}")
        cand &= np.isin(var_ids, want_v)
    on_gpu = engine_factory is None
    if on_gpu:
        from ._lib import LdEngine
        from .assoc import require_device
        require_device("seqFitLDpruning")
        engine_factory = LdEngine
    if verbose:
        print(f"LD pruning: {n_samp:,} samples, {M:,} variants, r^2 > {t2:g}, window {slide_max_bp:,} bp"
              + (f" / {slide_max_n} variants" if slide_max_n is not None else ""))
    step = max(1, _PASS_BYTES // max(nb, 1))
    kept_by_chrom: Dict[str, List] = {}
    eng = engine_factory(n_samp, nb)
    try:
        for r0, r1, name in chromosome_runs(chrom):
            if autosome_only and not _is_autosome(name):
                continue
            if np.any(np.diff(position[r0:r1]) < 0):
                raise ValueError(f"seqFitLDpruning: positions decrease within chromosome '{name}' (variants {r0}..{r1 - 1}).")
            run = _Run(eng, t2, int(slide_max_bp), None if slide_max_n is None else int(slide_max_n), int(block))
            n_cand = 0
            for v0 in range(r0, r1, step):
                v1 = min(r1, v0 + step)
                loc = np.flatnonzero(cand[v0:v1])
                if loc.size == 0:
                    continue
                rows = reader.read(v0, v1)
                if loc.size < v1 - v0:
                    rows = np.ascontiguousarray(rows[loc])
                nv, ac = _counts(rows, n_samp, on_gpu)
                ok = _marker_filter(nv, ac, n_samp, maf, missing_rate) & (ac > 0) & (ac < 2 * nv)      # (monomorphic: never)
                pick = np.flatnonzero(ok)
                n_cand += pick.size
                run.add(rows[pick], position[v0:v1][loc[pick]], var_ids[v0:v1][loc[pick]])
            kept = run.finish()
            kept_by_chrom.setdefault(name, []).extend(kept)
            if verbose:
                print(f"    chromosome {name}: {len(kept):,} of {n_cand:,} candidates kept")
    finally:
        if hasattr(eng, "close"):
            eng.close()
    out = {c: np.asarray(v, dtype=var_ids.dtype) for c, v in kept_by_chrom.items()}
    if save_gdsfn:
        _export(src, reader, out, var_ids, chrom, position, n_samp, [gsid[i] for i in sel], save_gdsfn, step)
    return out


def _export(src, reader: _Rows, kept: Dict[str, np.ndarray], var_ids, chrom, position, n_samp, sample_id, fn, step):
    """The kept variants as a SeqArray genotype file, in file order."""
    from .gds_write import write_seqarray_genotypes
    keep = np.flatnonzero(np.isin(var_ids, np.concatenate(list(kept.values())) if kept else np.zeros(0, var_ids.dtype)))
    parts = []
    for v0 in range(0, var_ids.size, step):
        loc = keep[(keep >= v0) & (keep < v0 + step)]
        if loc.size:
            parts.append(reader.read(v0, min(var_ids.size, v0 + step))[loc - v0])
    packed = np.concatenate(parts) if parts else np.zeros((0, reader.nb), dtype=np.uint8)
    if isinstance(src, GenotypeSource):
        allele = [f"{src.ref[i]},{src.alt[i]}" for i in keep]
    else:
        al = src.read("allele")
        allele = [str(al[i]) for i in keep]
    write_seqarray_genotypes(fn, packed, n_samp, sample_id=sample_id, variant_id=var_ids[keep], position=position[keep],
                             chromosome=[chrom[i] for i in keep], allele=allele)
