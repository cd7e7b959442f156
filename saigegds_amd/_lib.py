"""ctypes binding of libsaigehip.so (include/saigehip.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is
visible, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAIGEHIP_LIB") or os.path.join(_HERE, "libsaigehip.so")   # (the override: A/B runs of two builds)

GRM_MAX_RHS = 64      # SGX_GRM_MAX_RHS: columns of one batched GRM call
GRM_MAX_GROUPS = 64   # SGX_GRM_MAX_GROUPS: marker groups of one GRM handle
KMAT_WAVE_ROW = 33    # SGX_KMAT_WAVE_ROW: CSR rows of sgx_kmat with at least this many entries take the wave form
ENOSPACE = -5         # SGX_ENOSPACE: sgx_grm_sparse found more entries than the buffers hold
SKAT_MAX_VARIANTS = 4096   # SGX_SKAT_MAX_VARIANTS: entries of one unit of sgx_skat_2bit
SKATO_MAX_M = 256     # SGX_SKATO_MAX_M: order of one matrix of sgx_skato_spectra
COND_MAX = 16         # SGX_COND_MAX: conditioning variants of one sgx_cond_set
LD_BLOCK = 256        # SGX_LD_BLOCK: candidate rows of one sgx_ld_block_2bit call
TS_SLAB = 1024        # SGX_TS_SLAB: rows per partial of the tall-skinny Gram kernel (GrmOperator.ts_gram)
ERANK = -6            # SGX_ERANK: sgx_grm_pca's block of vectors lost rank
LD_MAX_ROWS = 4096    # SGX_LD_MAX_ROWS: rows a side of one sgx_ld_counts_2bit call
DS_MAX_COLS = 64      # SGX_DS_MAX_COLS: weight columns of one sgx_dsblock_burden call
DS_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float64): 2}   # SGX_DS_U8 / _I32 / _F64
# SGX_PR_*: the GDS classes whose rows cross PCIe as stored (sgx_scan_packed) and the numpy type of their values
PACKED_CLASSES = {"dPackedReal8U": 0, "dPackedReal8": 1, "dPackedReal16U": 2, "dPackedReal16": 3, "dFloat32": 4}
PACKED_DTYPES = (np.dtype(np.uint8), np.dtype(np.int8), np.dtype("<u2"), np.dtype("<i2"), np.dtype("<f4"))


def _packed_args(raw, cls, n, sel):
    """Checks of the shapes ctypes cannot see -> (raw, SGX_PR_* code, sel or None); the values are checked in C."""
    if isinstance(cls, str) and cls not in PACKED_CLASSES:
        raise ValueError(f"unknown packed-real class {cls!r}")
    code = PACKED_CLASSES[cls] if isinstance(cls, str) else int(cls)
    if 0 <= code < len(PACKED_DTYPES):
        raw = np.ascontiguousarray(raw, dtype=PACKED_DTYPES[code])
    else:
        raw = np.ascontiguousarray(raw)                # (an unknown code: the library refuses it)
    if raw.ndim != 2:
        raise ValueError("packed-real rows must be [n_variants, n_file_samp]")
    if sel is not None:
        sel = np.ascontiguousarray(sel)
        if sel.shape != (n,):
            raise ValueError(f"Invalid length of dosages: {sel.size}.")
        sel = np.clip(sel, -1, np.iinfo(np.int32).max).astype(np.int32)     # (out of int32's range stays out of range)
    return raw, code, sel


def _dbit2_args(alleles, bit0, n_file_samp, n_rows, sel, n, n_variants):
    """Checks of the sizes ctypes cannot see -> (alleles, n_rows or None, sel or None, m); the values are checked in C."""
    a = np.frombuffer(alleles, dtype=np.uint8) if not isinstance(alleles, np.ndarray) else alleles
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if n_rows is not None:
        n_rows = np.ascontiguousarray(np.clip(n_rows, -1, np.iinfo(np.int32).max), dtype=np.int32).reshape(-1)
        if n_variants is not None and int(n_variants) != n_rows.size:
            raise ValueError("n_rows must hold one count per variant")
        m, rows = n_rows.size, int(np.clip(n_rows, 0, None).sum(dtype=np.int64))
    else:
        if n_variants is None:
            raise ValueError("give n_variants or n_rows")
        m = rows = int(n_variants)
    if a.size < (int(bit0) + rows * int(n_file_samp) * 4 + 7) // 8:
        raise ValueError("allele buffer too short")
    if sel is not None:
        sel = np.ascontiguousarray(sel)
        if sel.shape != (n,):
            raise ValueError(f"Invalid length of dosages: {sel.size}.")
        sel = np.clip(sel, -1, np.iinfo(np.int32).max).astype(np.int32)     # (out of int32's range stays out of range)
    return a, n_rows, sel, m


class SgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsaigehip error {code}: {msg}")
        self.code = code


class PcaRankError(ValueError):
    """What an operator's ``pca`` raises when its block of vectors loses rank; ``seqFitPCA`` catches this type."""


class SgxRankError(SgxError, PcaRankError):
    """``sgx_grm_pca``: the block of vectors lost rank (SGX_ERANK)."""


class SgxModel(C.Structure):
    _fields_ = [
        ("n_samp", C.c_int32), ("n_coeff", C.c_int32), ("trait", C.c_int32), ("reserved", C.c_int32),
        ("tau", C.c_double * 2), ("var_ratio", C.c_double),
        ("maf", C.c_double), ("mac", C.c_double), ("missing", C.c_double), ("spa_pval", C.c_double),
        ("y", C.c_void_p), ("mu", C.c_void_p), ("y_mu", C.c_void_p), ("mu2", C.c_void_p),
        ("t_XXVX_inv", C.c_void_p), ("XV", C.c_void_p), ("t_XVX_inv_XV", C.c_void_p),
        ("XVX", C.c_void_p), ("t_X", C.c_void_p), ("S_a", C.c_void_p),
    ]


class SgxStats(C.Structure):
    _fields_ = [
        ("n_variants", C.c_uint64), ("n_valid", C.c_uint64), ("n_spa", C.c_uint64),
        ("n_spa_dense", C.c_uint64), ("n_spa_slow", C.c_uint64),
        ("ms_score", C.c_float), ("ms_spa", C.c_float), ("ms_total", C.c_float),
        ("score_launches", C.c_uint32), ("spa_launches", C.c_uint32), ("ms_kernel", C.c_float),
        ("ms_lists", C.c_float), ("three_plane", C.c_uint32), ("n_unlisted", C.c_uint32), ("n_guarded", C.c_uint32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SgxGrmSparseStats(C.Structure):
    _fields_ = [
        ("tiles_screened", C.c_int64), ("subtiles_total", C.c_int64), ("subtiles_flagged", C.c_int64),
        ("entries", C.c_int64), ("s", C.c_int32), ("reserved", C.c_int32),
        ("ms_prepare", C.c_double), ("ms_screen", C.c_double), ("ms_fp64", C.c_double), ("ms_sort", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class SgxGrmKingStats(C.Structure):
    _fields_ = [("tiles", C.c_int64), ("pairs", C.c_int64), ("ms_kernel", C.c_double), ("ms_sort", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SgxGrmPcaStats(C.Structure):
    _fields_ = [("iters", C.c_int32), ("n_converged", C.c_int32), ("ms_products", C.c_double), ("ms_block", C.c_double)]


def _abi():
    """include/saigehip.h as ctypes: every exported function -> (restype, argtypes; None: takes no argument)."""
    vp, sz, dp, ci, i32, ll, u64, ptr = (C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_int32, C.c_longlong, C.c_uint64,
                                         C.POINTER)
    pvp = ptr(vp)
    return {
        "sgx_version": (C.c_char_p, None),
        "sgx_last_error": (C.c_char_p, None),
        "sgx_device_count": (ci, None),
        "sgx_init": (ci, [ptr(SgxModel), ci, pvp]),
        "sgx_free": (None, [vp]),
        "sgx_set_thresholds": (ci, [vp, dp, dp, dp, dp]),
        "sgx_score_layout": (ci, [vp, vp, i32, ptr(i32)]),
        "sgx_scan_2bit": (ci, [vp, vp, sz, sz, vp, vp]),
        "sgx_scan_2bit_dev": (ci, [vp, vp, sz, sz, vp, vp]),
        "sgx_scan_u8": (ci, [vp, vp, sz, vp, vp]),
        "sgx_scan_i32": (ci, [vp, vp, sz, vp, vp]),
        "sgx_scan_f64": (ci, [vp, vp, sz, vp, vp]),
        "sgx_host_alloc": (vp, [sz]),
        "sgx_host_free": (None, [vp]),
        "sgx_live_bytes": (sz, None),
        "sgx_burden_2bit": (ci, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "sgx_geno_stats_2bit": (ci, [vp, sz, i32, sz, ci, vp, vp]),
        "sgx_decode_dbit2": (ci, [vp, sz, i32, sz, vp, i32, vp, sz, ci]),
        "sgx_block_bytes": (sz, [i32, sz]),
        "sgx_block_create": (ci, [i32, sz, ci, pvp]),
        "sgx_block_create_ex": (ci, [i32, sz, ci, ll, pvp]),
        "sgx_block_free": (None, [vp]),
        "sgx_block_load_dev": (ci, [vp, vp, vp, sz, sz]),
        "sgx_block_load": (ci, [vp, vp, vp, sz, sz]),
        "sgx_block_variants": (sz, [vp]),
        "sgx_scan_block": (ci, [vp, vp, vp, vp]),
        "sgx_sync": (ci, [vp]),
        "sgx_get_stats": (ci, [vp, ptr(SgxStats)]),
        "sgx_get_stats_total": (ci, [vp, ptr(SgxStats), ptr(u64), ci]),
        "sgx_row_stride": (sz, [i32]),
        "sgx_synth_2bit_dev": (ci, [vp, vp, sz, i32, sz, u64, u64, vp]),
        "sgx_selftest": (ci, [ci]),
        "sgx_set_option": (ci, [vp, C.c_char_p, ll]),
        "sgx_grm_init": (ci, [vp, sz, i32, sz, ci, pvp]),
        "sgx_grm_init_dev": (ci, [vp, sz, i32, sz, ci, pvp]),
        "sgx_grm_crossprod_dev": (ci, [vp, vp, vp]),
        "sgx_grm_sync": (ci, [vp]),
        "sgx_grm_free": (None, [vp]),
        "sgx_grm_diag": (ci, [vp, vp]),
        "sgx_grm_crossprod": (ci, [vp, vp, vp]),
        "sgx_grm_pcg": (ci, [vp, vp, vp, vp, ci, dp, vp, ptr(ci)]),
        "sgx_grm_crossprod_multi": (ci, [vp, vp, sz, ci, vp]),
        "sgx_grm_crossprod_multi_dev": (ci, [vp, vp, sz, ci, vp]),
        "sgx_grm_pcg_multi": (ci, [vp, vp, vp, vp, sz, ci, ci, dp, vp, vp]),
        "sgx_grm_set_groups": (ci, [vp, vp, ci]),
        "sgx_grm_group_sizes": (ci, [vp, vp]),
        "sgx_grm_diag_loco": (ci, [vp, ci, vp]),
        "sgx_grm_crossprod_loco": (ci, [vp, vp, sz, ci, vp, vp]),
        "sgx_grm_pcg_loco": (ci, [vp, vp, sz, ci, vp, vp, vp, sz, ci, vp, ci, dp, vp, vp]),
        "sgx_grm_dense": (ci, [vp, i32, i32, i32, i32, vp, sz]),
        "sgx_grm_dense_kernel_ms": (ci, [vp, ptr(dp)]),
        "sgx_grm_sparse": (ci, [vp, dp, sz, vp, vp, vp, ptr(sz), ptr(SgxGrmSparseStats)]),
        "sgx_grm_marker_table": (ci, [vp, vp, vp]),
        "sgx_grm_marker_dots": (ci, [vp, vp, sz, ci, vp, sz]),
        "sgx_grm_marker_dots_dev": (ci, [vp, vp, sz, ci, vp, sz]),
        "sgx_grm_pca": (ci, [vp, ci, ci, vp, sz, ci, dp, vp, vp, vp, sz, vp, sz, ptr(SgxGrmPcaStats)]),
        "sgx_grm_ts_gram": (ci, [vp, i32, vp, sz, ci, vp, sz, ci, vp]),
        "sgx_grm_ts_apply": (ci, [vp, i32, vp, sz, ci, vp, ci, vp, sz]),
        "sgx_grm_king_counts": (ci, [vp, i32, i32, i32, i32, vp, sz]),
        "sgx_grm_king_pairs": (ci, [vp, dp, sz, vp, vp, vp, vp, vp, ptr(sz), ptr(SgxGrmKingStats)]),
        "sgx_kmat_init_csr": (ci, [i32, vp, vp, vp, ci, pvp]),
        "sgx_kmat_init_dense": (ci, [vp, sz, i32, ci, pvp]),
        "sgx_kmat_free": (None, [vp]),
        "sgx_kmat_sync": (ci, [vp]),
        "sgx_kmat_diag": (ci, [vp, vp]),
        "sgx_kmat_crossprod_multi": (ci, [vp, vp, sz, ci, vp]),
        "sgx_kmat_crossprod_multi_dev": (ci, [vp, vp, sz, ci, vp]),
        "sgx_kmat_pcg_multi": (ci, [vp, vp, vp, vp, sz, ci, ci, dp, vp, vp]),
        "sgx_kmat_matvec_ms": (ci, [vp, ptr(dp)]),
        "sgx_kmat_pcg_multi_dev": (ci, [vp, vp, vp, vp, sz, ci, ci, dp, vp, vp]),
        "sgx_skat_kmat_2bit": (ci, [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, ci, dp, vp, vp, vp]),
        "sgx_skat_kmat_ms": (ci, [vp, vp]),
        "sgx_cond_kmat_set": (ci, [vp, vp, vp, sz, sz, vp, vp, vp, ci, dp, vp, vp, vp]),
        "sgx_cond_kmat_2bit": (ci, [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]),
        "sgx_dsblock_create": (ci, [i32, ci, sz, ci, pvp]),
        "sgx_dsblock_free": (None, [vp]),
        "sgx_dsblock_load": (ci, [vp, vp, vp, sz, vp, vp, vp]),
        "sgx_dsblock_scan": (ci, [vp, vp, vp, vp]),
        "sgx_dsblock_burden": (ci, [vp, vp, sz, vp, vp, vp, ci, vp, vp, vp, vp]),
        "sgx_scan_packed": (ci, [vp, vp, ci, sz, dp, dp, vp, sz, vp, vp]),
        "sgx_ds_block_load_packed": (ci, [vp, vp, vp, ci, sz, dp, dp, vp, sz, vp, vp, vp]),
        "sgx_scan_dbit2": (ci, [vp, vp, sz, sz, vp, vp, sz, vp, vp]),
        "sgx_block_load_dbit2": (ci, [vp, vp, vp, sz, sz, vp, vp, sz]),
        "sgx_quantize_packed": (ci, [vp, ci, sz, dp, dp, vp, i32, sz, ci, sz, vp, sz, vp, vp, vp, vp]),
        "sgx_skat_2bit": (ci, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "sgx_ds_block_skat": (ci, [vp, vp, sz, vp, vp, vp, vp, vp, vp]),
        "sgx_cond_set": (ci, [vp, vp, sz, sz, vp, vp, vp]),
        "sgx_cond_2bit": (ci, [vp, vp, sz, sz, vp, vp, vp, vp]),
        "sgx_cond_2bit_dev": (ci, [vp, vp, sz, sz, vp, vp, vp, vp]),
        "sgx_firth_2bit": (ci, [vp, vp, sz, sz, vp, ci, vp]),
        "sgx_firth_2bit_dev": (ci, [vp, vp, sz, sz, vp, ci, vp]),
        "sgx_exact_2bit": (ci, [vp, vp, sz, sz, vp, ci, vp]),
        "sgx_exact_2bit_dev": (ci, [vp, vp, sz, sz, vp, ci, vp]),
        "sgx_ds_block_cond_set": (ci, [vp, vp, sz, vp, vp, vp, vp, vp]),
        "sgx_ds_block_cond": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "sgx_ds_block_firth": (ci, [vp, vp, sz, vp, vp, vp, ci, vp]),
        "sgx_ds_block_skat_kmat": (ci, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, dp, vp, vp, vp]),
        "sgx_ds_block_cond_kmat_set": (ci, [vp, vp, vp, sz, vp, vp, vp, vp, vp, ci, dp, vp, vp, vp]),
        "sgx_ds_block_cond_kmat": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgx_skato_spectra": (ci, [vp, sz, vp, vp, sz, vp, vp, vp]),
        "sgx_collapse_2bit": (ci, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "sgx_collapse_2bit_dev": (ci, [vp, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "sgx_ds_block_collapse": (ci, [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sgx_ld_create": (ci, [ci, i32, sz, sz, pvp]),
        "sgx_ld_free": (None, [vp]),
        "sgx_ld_counts_2bit": (ci, [vp, vp, sz, vp, sz, vp]),
        "sgx_ld_block_2bit": (ci, [vp, vp, sz, dp, vp]),
        "sgx_ld_window_push": (ci, [vp, vp, sz, sz]),
        "sgx_ld_window_reset": (ci, [vp]),
        "sgx_ld_window_len": (C.c_int64, [vp]),
        "sgx_ld_kernel_ms": (ci, [vp, ptr(dp)]),
    }


ABI = _abi()
EXPORTS = tuple(ABI)

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so.  Two HIP runtimes in one
    process cannot both open the GPU, so when torch is installed its copy is
    loaded first; libsaigehip.so (NEEDED libamdhip64.so.7) then binds to it by
    SONAME.  Without torch (e.g. under R) the system ROCm runtime is used."""
    if os.environ.get("SAIGEHIP_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def load():
    """Load libsaigehip.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C saigegds_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        f = getattr(L, name)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    _lib = L
    return L


def live_bytes() -> int:
    """Device and pinned bytes the library holds in this process (``sgx_live_bytes``); 0 once every object is closed."""
    return int(load().sgx_live_bytes())


def check(rc: int):
    if rc != 0:
        raise SgxError(rc, load().sgx_last_error().decode("utf-8", "replace"))


class _Handle:
    """An object the library made: the attribute ``_attr`` holds it, the function ``_free`` releases it.  ``close()``
    may come any number of times; ``with`` and the collector close too."""

    _attr, _free = "_h", None
    _L = property(lambda self: load())

    def close(self):
        if getattr(self, self._attr, None):
            getattr(self._L, self._free)(getattr(self, self._attr))
            setattr(self, self._attr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _csr_ptr(what: str, msg: str, ptr, var_idx: np.ndarray, entries, ok: bool = True):
    """The shape checks of a CSR ``ptr`` over the entries ``var_idx`` (``entries``: the per-entry arrays, each with the
    shape of one entry; ``ok``: the caller's own condition) -> (ptr int64, the number of its groups)."""
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    n = ptr.size - 1
    if not ok or any(a.shape != (var_idx.size,) + one for a, one in entries) or n < 0 or ptr[-1] != var_idx.size:
        raise ValueError(f"{what}: {msg}")
    return ptr, n


def _unit_args(what: str, unit_ptr, var_idx, entries, ok: bool = True):
    """Checks of the set tests' units (CSR ``unit_ptr`` / ``var_idx`` over rows; ``entries`` and ``ok`` as for
    ``_csr_ptr``) -> (unit_ptr int64, var_idx int32, n_units, the units' sizes m, the offsets of their m x m matrices in
    one buffer)."""
    var_idx = np.ascontiguousarray(var_idx, dtype=np.int32)
    unit_ptr, n_units = _csr_ptr(what, "inconsistent CSR / table shapes", unit_ptr, var_idx, entries, ok and var_idx.ndim == 1)
    sizes = np.diff(unit_ptr)
    if (sizes < 0).any():
        raise ValueError(f"{what}: unit_ptr not ascending")
    return unit_ptr, var_idx, n_units, sizes, np.concatenate([[0], np.cumsum(sizes * sizes)])


def _unit_matrices(cov: np.ndarray, sizes, offs):
    """The buffer of all units' matrices -> per unit an [m, m] view."""
    return [cov[offs[u]:offs[u + 1]].reshape(sizes[u], sizes[u]) for u in range(sizes.size)]


def _row_tables(what: str, packed, lut, per: str = "row"):
    """2-bit rows with one 4-entry dosage table each -> (packed uint8, lut float64 [m, 4])."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    lut = np.ascontiguousarray(lut, dtype=np.float64).reshape(-1, 4)
    if packed.ndim != 2 or lut.shape[0] != packed.shape[0]:
        raise ValueError(f"{what}: one table per {per}")
    return packed, lut


def _flip_mean(what: str, msg: str, flip, mean, var_idx=None, n: int = 0):
    """``flip`` / ``mean`` of the entries on a dosage block, one per entry of ``var_idx`` or, without it, ``n`` of each
    -> (flip uint8, mean float64, var_idx int32)."""
    flip = np.ascontiguousarray(flip, dtype=np.uint8)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    if var_idx is not None:
        var_idx = np.ascontiguousarray(var_idx, dtype=np.int32)
    shape = (n,) if var_idx is None else var_idx.shape
    if len(shape) != 1 or flip.shape != shape or mean.shape != shape:
        raise ValueError(f"{what}: {msg}")
    return flip, mean, var_idx


def _sigma_args(what: str, op, w, tau):
    """``w`` [samples of the matrix] and ``tau`` [2] of the entries on an explicit GRM, as float64."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    if w.shape != (op.n,) or tau.shape != (2,):
        raise ValueError(f"{what}: w must have one entry per sample of the matrix and tau two entries")
    return w, tau


class Scanner(_Handle):
    """One model resident on one GPU (an ``sgx_handle``)."""

    _free = "sgx_free"
    ds_collapse = True      # its dosage blocks have ``collapse``: what ``collapse_mac=`` on dosage input asks of a scanner class

    def __init__(self, sm, device: int = 0):
        L = load()
        self.n, self.k, self.quant = sm.n, sm.k, sm.quant
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        self._keep = dict(y=f(sm.y), mu=f(sm.mu), y_mu=f(sm.y_mu), mu2=f(sm.mu2),
                          t_XXVX_inv=f(sm.t_XXVX_inv), XV=f(sm.XV), t_XVX_inv_XV=f(sm.t_XVX_inv_XV),
                          XVX=f(sm.XVX), t_X=f(sm.t_X), S_a=f(sm.S_a))
        m = SgxModel()
        m.n_samp, m.n_coeff = sm.n, sm.k
        m.trait = 1 if sm.quant else 0
        m.tau[0], m.tau[1] = float(sm.tau[0]), float(sm.tau[1])
        m.var_ratio = sm.var_ratio
        m.maf, m.mac, m.missing, m.spa_pval = sm.maf, sm.mac, sm.missing, sm.spa_pval
        for k, a in self._keep.items():
            setattr(m, k, a.ctypes.data)
        h = C.c_void_p()
        check(L.sgx_init(C.byref(m), int(device), C.byref(h)))
        self._h = h
        self.device = device

    # -- host-buffer scans -------------------------------------------------
    def _out(self, m):
        return np.empty((m, 8), dtype=np.float64), np.zeros(m, dtype=np.uint8)

    def scan_2bit(self, packed: np.ndarray):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        if packed.ndim != 2:
            raise ValueError("packed genotypes must be [n_variants, bytes_per_variant]")
        m, bpv = packed.shape
        out, valid = self._out(m)
        check(self._L.sgx_scan_2bit(self._h, packed.ctypes.data, bpv, m, out.ctypes.data,
                                    valid.ctypes.data))
        return out, valid

    def _scan_dosage(self, dosage, dtype, entry: str):
        dosage = np.ascontiguousarray(dosage, dtype=dtype)
        if dosage.ndim != 2 or dosage.shape[1] != self.n:
            raise ValueError(f"Invalid length of dosages: {dosage.shape[-1]}.")
        out, valid = self._out(dosage.shape[0])
        check(getattr(self._L, entry)(self._h, dosage.ctypes.data, dosage.shape[0], out.ctypes.data, valid.ctypes.data))
        return out, valid

    def scan_u8(self, dosage: np.ndarray):
        return self._scan_dosage(dosage, np.uint8, "sgx_scan_u8")

    def scan_i32(self, dosage: np.ndarray):
        """INTEGER dosages, NA_INTEGER (-2147483648) = missing (the INTSXP branch of get_ds)."""
        return self._scan_dosage(dosage, np.int32, "sgx_scan_i32")

    def scan_f64(self, dosage: np.ndarray):
        return self._scan_dosage(dosage, np.float64, "sgx_scan_f64")

    def scan_packed(self, raw: np.ndarray, cls, scale: float, offset: float, sel=None):
        """Packed-real dosage rows as the file stores them (``sgx_scan_packed``): ``raw`` [m, n_file_samp] integers
        (or float32) of class ``cls`` (a GDS class name or an SGX_PR_* code), dosage = raw * scale + offset, decoded
        on the device.  ``sel``: None (the file's samples are the model's) or the model's samples as indices into
        the file's.  Equals ``scan_f64`` of the decoded, selected rows bit for bit."""
        raw, code, sel = _packed_args(raw, cls, self.n, sel)
        out, valid = self._out(raw.shape[0])
        check(self._L.sgx_scan_packed(self._h, raw.ctypes.data, code, raw.shape[1], float(scale), float(offset),
                                      None if sel is None else sel.ctypes.data, raw.shape[0], out.ctypes.data,
                                      valid.ctypes.data))
        return out, valid

    def scan_dbit2(self, alleles, bit0: int, n_file_samp: int, n_rows=None, sel=None, n_variants: int = None):
        """``genotype/data`` rows as the file stores them (``sgx_scan_dbit2``; ``GdsFile.genotype_raw_range``): the
        bytes that hold the variants' dBit2 rows from bit ``bit0`` of the first byte on, ``n_file_samp`` samples a row.
        ``n_rows``: None (one row per variant, ``n_variants`` of them) or the rows of each variant.  ``sel``: None (the
        file's samples are the model's) or the model's samples as indices into the file's.  Decoded on the device;
        equals ``scan_2bit`` of ``decode_dbit2``'s rows bit for bit."""
        a, n_rows, sel, m = _dbit2_args(alleles, bit0, n_file_samp, n_rows, sel, self.n, n_variants)
        out, valid = self._out(m)
        check(self._L.sgx_scan_dbit2(self._h, a.ctypes.data, int(bit0), int(n_file_samp),
                                     None if n_rows is None else n_rows.ctypes.data, None if sel is None else sel.ctypes.data,
                                     m, out.ctypes.data, valid.ctypes.data))
        return out, valid

    def burden_2bit(self, packed: np.ndarray, row_ptr, var_idx, lut):
        """Burden rows (CSR over the rows of ``packed``, one 4-entry table per entry), then the
        single-variant test on each row (``sgx_burden_2bit``)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        var_idx = np.ascontiguousarray(var_idx, dtype=np.int32)
        lut = np.ascontiguousarray(lut, dtype=np.float64)
        row_ptr, n_rows = _csr_ptr("burden_2bit", "inconsistent CSR / table shapes", row_ptr, var_idx, [(lut, (4,))],
                                   packed.ndim == 2)
        out, valid = self._out(n_rows)
        check(self._L.sgx_burden_2bit(self._h, packed.ctypes.data, packed.shape[1], packed.shape[0], n_rows,
                                      row_ptr.ctypes.data, var_idx.ctypes.data, lut.ctypes.data,
                                      out.ctypes.data, valid.ctypes.data))
        return out, valid

    def skat_2bit(self, packed: np.ndarray, unit_ptr, var_idx, lut):
        """Score statistics and their covariance per unit (CSR over the rows of ``packed``, one 4-entry dosage table
        per entry; ``sgx_skat_2bit``) -> (score [entries], cov: per unit an [m, m] symmetric matrix)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lut = np.ascontiguousarray(lut, dtype=np.float64).reshape(-1, 4)
        unit_ptr, var_idx, n_units, sizes, offs = _unit_args("skat_2bit", unit_ptr, var_idx, [(lut, (4,))], packed.ndim == 2)
        score, cov = np.zeros(max(1, var_idx.size)), np.zeros(max(1, int(offs[-1])))
        if var_idx.size:
            check(self._L.sgx_skat_2bit(self._h, packed.ctypes.data, packed.shape[1], packed.shape[0], n_units,
                                        unit_ptr.ctypes.data, var_idx.ctypes.data, lut.ctypes.data,
                                        score.ctypes.data, cov.ctypes.data))
        return score[:var_idx.size], _unit_matrices(cov, sizes, offs)

    def skat_kmat(self, op, packed: np.ndarray, unit_ptr, var_idx, lut, w, tau, maxiter: int = 500, tol: float = 1e-5):
        """``skat_2bit`` with the covariance under the fitted model on the explicit GRM of ``op`` (an
        ``ExplicitGrmOperator`` on this scanner's device): ``Phi^K = A' P A`` with ``Sigma = tau[0] diag(1/w) +
        tau[1] K`` (``sgx_skat_kmat_2bit``) -> (score [entries], cov: per unit an [m, m] symmetric matrix,
        iters [entries]: PCG steps of every entry's solve)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lut = np.ascontiguousarray(lut, dtype=np.float64).reshape(-1, 4)
        unit_ptr, var_idx, n_units, sizes, offs = _unit_args("skat_kmat", unit_ptr, var_idx, [(lut, (4,))], packed.ndim == 2)
        w, tau = _sigma_args("skat_kmat", op, w, tau)
        score, cov = np.zeros(max(1, var_idx.size)), np.zeros(max(1, int(offs[-1])))
        iters = np.zeros(max(1, var_idx.size), dtype=np.int32)
        if var_idx.size:
            check(self._L.sgx_skat_kmat_2bit(self._h, op._h, packed.ctypes.data, packed.shape[1], packed.shape[0], n_units,
                                             unit_ptr.ctypes.data, var_idx.ctypes.data, lut.ctypes.data, w.ctypes.data,
                                             tau.ctypes.data, int(maxiter), float(tol), score.ctypes.data, cov.ctypes.data,
                                             iters.ctypes.data))
        return score[:var_idx.size], _unit_matrices(cov, sizes, offs), iters[:var_idx.size]

    def skat_kmat_ms(self) -> np.ndarray:
        """Host milliseconds of the last ``skat_kmat`` call: columns, solves, products."""
        ms = np.zeros(3)
        check(self._L.sgx_skat_kmat_ms(self._h, ms.ctypes.data))
        return ms

    def skato_spectra(self, mats, rho):
        """The SKAT-O null eigenvalues of a batch of units (``sgx_skato_spectra``): ``mats`` a list of symmetric [m, m]
        matrices ``A = diag(w) Phi diag(w)`` (m up to ``SKATO_MAX_M``), ``rho`` the grid shared by all -> (per problem
        an array [len(rho) + 1, m]: row k the eigenvalues of ``B_rho[k]`` ascending, the last row those of ``W = A -
        r r' / c``, not clipped; sweeps [n, len(rho) + 1] int32: Jacobi sweeps that rotated, -1 where the matrix held a
        non-finite entry and its eigenvalues are NaN)."""
        mats = [np.ascontiguousarray(a, dtype=np.float64) for a in mats]
        if any(a.ndim != 2 or a.shape[0] != a.shape[1] for a in mats):
            raise ValueError("skato_spectra: every problem must be a square matrix")
        rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        n, nmat = len(mats), rho.size + 1
        m = np.array([a.shape[0] for a in mats], dtype=np.int32)
        flat = np.concatenate([a.ravel() for a in mats]) if n else np.zeros(0)
        flat = np.ascontiguousarray(flat) if flat.size else np.zeros(1)
        eig = np.zeros(max(1, nmat * int(m.sum(dtype=np.int64))))
        sweeps = np.zeros((max(1, n), nmat), dtype=np.int32)
        check(self._L.sgx_skato_spectra(self._h, n, m.ctypes.data if n else None, flat.ctypes.data, rho.size,
                                        rho.ctypes.data if rho.size else None, eig.ctypes.data, sweeps.ctypes.data))
        offs = np.concatenate([[0], np.cumsum(m.astype(np.int64) * nmat)])
        return [eig[offs[u]:offs[u + 1]].reshape(nmat, m[u]) for u in range(n)], sweeps[:n]

    def cond_set(self, packed_c: np.ndarray, lut_c):
        """Installs the conditioning set of the conditional scan (``sgx_cond_set``): its 2-bit rows and 4-entry dosage
        tables -> (score_c [C], cov_cc [C, C]), which equal ``skat_2bit`` on the rows as one unit bit for bit.  No rows
        clears the set."""
        packed_c, lut_c = _row_tables("cond_set", packed_c, lut_c, "conditioning row")
        c = packed_c.shape[0]
        score, cov = np.zeros(max(1, c)), np.zeros(max(1, c * c))
        check(self._L.sgx_cond_set(self._h, packed_c.ctypes.data, packed_c.shape[1], c, lut_c.ctypes.data,
                                   score.ctypes.data, cov.ctypes.data))
        self._n_cond = c
        return score[:c], cov[:c * c].reshape(c, c)

    def cond_2bit(self, packed: np.ndarray, lut):
        """Score, variance and covariances with the installed conditioning set of every 2-bit row (one 4-entry dosage
        table each; ``sgx_cond_2bit``) -> (score [m], var [m], cov [m, C])."""
        packed, lut = _row_tables("cond_2bit", packed, lut)
        m, c = packed.shape[0], getattr(self, "_n_cond", 0)
        score, var, cov = np.zeros(m), np.zeros(m), np.zeros((m, max(1, c)))
        check(self._L.sgx_cond_2bit(self._h, packed.ctypes.data, packed.shape[1], m, lut.ctypes.data,
                                    score.ctypes.data, var.ctypes.data, cov.ctypes.data))
        return score, var, cov[:, :c]

    def cond_kmat_set(self, op, packed_c: np.ndarray, lut_c, w, tau, maxiter: int = 500, tol: float = 1e-5):
        """Installs the conditioning set of the conditional scan on the explicit GRM of ``op`` (an ``ExplicitGrmOperator``
        on this scanner's device; ``sgx_cond_kmat_set``): rows, tables, ``w`` and ``tau`` as for ``skat_kmat`` ->
        (S_C [C], Phi^K_CC [C, C], iters [C]), which equal ``skat_kmat`` on the rows as one unit bit for bit.  No rows
        clears the set; the set of ``cond_set`` is not touched."""
        packed_c, lut_c = _row_tables("cond_kmat_set", packed_c, lut_c, "conditioning row")
        w, tau = _sigma_args("cond_kmat_set", op, w, tau)
        c = packed_c.shape[0]
        score, cov, iters = np.zeros(max(1, c)), np.zeros(max(1, c * c)), np.zeros(max(1, c), dtype=np.int32)
        check(self._L.sgx_cond_kmat_set(self._h, op._h, packed_c.ctypes.data, packed_c.shape[1], c, lut_c.ctypes.data,
                                        w.ctypes.data, tau.ctypes.data, int(maxiter), float(tol), score.ctypes.data,
                                        cov.ctypes.data, iters.ctypes.data))
        self._n_cond_kmat = c
        return score[:c], cov[:c * c].reshape(c, c), iters[:c]

    def cond_kmat(self, op, packed: np.ndarray, lut):
        """Score, variance and covariances with the set of ``cond_kmat_set`` of every 2-bit row under the fitted model on
        the explicit GRM (``sgx_cond_kmat_2bit``) -> (score [m], var [m], cov [m, C], iters [m]: PCG steps of the
        row's column)."""
        packed, lut = _row_tables("cond_kmat", packed, lut)
        m, c = packed.shape[0], getattr(self, "_n_cond_kmat", 0)
        score, var, cov, iters = np.zeros(m), np.zeros(m), np.zeros((m, max(1, c))), np.zeros(m, dtype=np.int32)
        check(self._L.sgx_cond_kmat_2bit(self._h, op._h, packed.ctypes.data, packed.shape[1], m, lut.ctypes.data,
                                         score.ctypes.data, var.ctypes.data, cov.ctypes.data, iters.ctypes.data))
        return score, var, cov[:, :c], iters

    def cond_2bit_dev(self, packed_ptr: int, bpv: int, m: int, lut_ptr: int, score_ptr: int, var_ptr: int, cov_ptr: int):
        """``cond_2bit`` on rows, tables and results in device memory (``sgx_cond_2bit_dev``; asynchronous, sync()
        before reading)."""
        check(self._L.sgx_cond_2bit_dev(self._h, packed_ptr, bpv, m, lut_ptr, score_ptr, var_ptr, cov_ptr))

    def _out4_2bit(self, what: str, packed, lut, opt: int):
        """``sgx_<what>`` on 2-bit rows with one table each and the entry's integer option -> out4 [m, 4]."""
        packed, lut = _row_tables(what, packed, lut)
        m = packed.shape[0]
        out4 = np.zeros((max(1, m), 4))
        check(getattr(self._L, "sgx_" + what)(self._h, packed.ctypes.data, packed.shape[1], m, lut.ctypes.data, int(opt),
                                              out4.ctypes.data))
        return out4[:m]

    def _out4_2bit_dev(self, what: str, packed_ptr: int, bpv: int, m: int, lut_ptr: int, opt: int, out4_ptr: int):
        """``sgx_<what>`` on rows, tables and out4 in device memory, with the entry's integer option."""
        check(getattr(self._L, "sgx_" + what)(self._h, packed_ptr, bpv, m, lut_ptr, int(opt), out4_ptr))

    def firth_2bit(self, packed: np.ndarray, lut, maxit: int = 50):
        """Firth bias-reduced effect size of every 2-bit row (one 4-entry dosage table each; ``sgx_firth_2bit``; binary
        traits) -> out4 [m, 4]: beta for the table's orientation, SE, iterations, converged (1 / 0).  NaN / NaN / 0 for a
        row without a non-zero dosage or with a non-finite table value."""
        return self._out4_2bit("firth_2bit", packed, lut, maxit)

    def firth_2bit_dev(self, packed_ptr: int, bpv: int, m: int, lut_ptr: int, out4_ptr: int, maxit: int = 50):
        """``firth_2bit`` on rows, tables and results in device memory (``sgx_firth_2bit_dev``; asynchronous, sync()
        before reading)."""
        self._out4_2bit_dev("firth_2bit_dev", packed_ptr, bpv, m, lut_ptr, maxit, out4_ptr)

    def exact_2bit(self, packed: np.ndarray, lut, max_mac: int):
        """Exact p-values of the 2-bit rows with at most ``max_mac`` (1..63) minor alleles (one 4-entry dosage table
        each; ``sgx_exact_2bit``; binary traits) -> out4 [m, 4]: p.mid, p.full, MAC, done (1 / 0).  NaN /
        NaN / MAC / 0 for a row with no carrier or more than ``max_mac`` minor alleles, NaN / NaN / 0 / 0 for a table
        that is not {0, 1, 2, finite} or {2, 1, 0, finite}."""
        return self._out4_2bit("exact_2bit", packed, lut, max_mac)

    def exact_2bit_dev(self, packed_ptr: int, bpv: int, m: int, lut_ptr: int, out4_ptr: int, max_mac: int):
        """``exact_2bit`` on rows, tables and results in device memory (``sgx_exact_2bit_dev``; asynchronous, sync()
        before reading)."""
        self._out4_2bit_dev("exact_2bit_dev", packed_ptr, bpv, m, lut_ptr, max_mac, out4_ptr)

    def collapse_2bit(self, packed: np.ndarray, grp_ptr, var_idx, flip):
        """The pseudo-variant of every group of 2-bit rows (CSR ``grp_ptr`` / ``var_idx`` over the rows of ``packed``, one
        flip byte per entry; ``sgx_collapse_2bit``): per sample the largest minor-allele dosage over the
        group's rows (the code, 2 - code where flipped, 0 where missing) -> (rows [n_groups, bpv] uint8 with codes 0, 1,
        2 and zero padding, counts [n_groups, 2] int32: samples with code 1 and with code 2)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        flip = np.ascontiguousarray(flip, dtype=np.uint8)
        grp_ptr, var_idx, n_groups, _, _ = _unit_args("collapse_2bit", grp_ptr, var_idx, [(flip, ())], packed.ndim == 2)
        rows, counts = np.zeros((n_groups, packed.shape[1]), dtype=np.uint8), np.zeros((n_groups, 2), dtype=np.int32)
        if var_idx.size:                              # (groups without an entry: the zeros above)
            check(self._L.sgx_collapse_2bit(self._h, packed.ctypes.data, packed.shape[1], packed.shape[0], n_groups,
                                            grp_ptr.ctypes.data, var_idx.ctypes.data, flip.ctypes.data, rows.ctypes.data,
                                            counts.ctypes.data))
        return rows, counts

    def collapse_2bit_dev(self, packed_ptr: int, bpv: int, m: int, n_groups: int, grp_ptr_ptr: int, var_idx_ptr: int,
                          flip_ptr: int, out_rows_ptr: int, counts_ptr: int):
        """``collapse_2bit`` on rows, groups and results in device memory (``sgx_collapse_2bit_dev``: the groups are
        checked on the host first, the kernel is asynchronous; sync() before reading)."""
        check(self._L.sgx_collapse_2bit_dev(self._h, packed_ptr, bpv, m, n_groups, grp_ptr_ptr, var_idx_ptr, flip_ptr,
                                            out_rows_ptr, counts_ptr))

    def dosage_block(self, dtype, max_variants: int) -> "DosageBlock":
        """Device storage for a batch of dosage rows of the aggregate tests (``DosageBlock`` below)."""
        return DosageBlock(self, dtype, max_variants)

    # -- device-resident scans (pointers are raw device addresses) ---------
    def row_stride(self) -> int:
        return int(self._L.sgx_row_stride(self.n))

    def scan_2bit_dev(self, packed_ptr: int, bpv: int, m: int, out_ptr: int, valid_ptr: int):
        check(self._L.sgx_scan_2bit_dev(self._h, packed_ptr, bpv, m, out_ptr, valid_ptr))

    # -- genotype blocks (rows + their sparse side resident on the device; Block below) ---
    def load_block_dev(self, block: "Block", packed_ptr: int, bpv: int, m: int):
        """Rows already in this GPU's memory -> block (asynchronous on the handle's stream)."""
        check(self._L.sgx_block_load_dev(self._h, block._b, packed_ptr, bpv, m))

    def load_block(self, block: "Block", packed: np.ndarray):
        """Rows in host memory -> block, through the pinned pipeline."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        if packed.ndim != 2:
            raise ValueError("packed genotypes must be [n_variants, bytes_per_variant]")
        check(self._L.sgx_block_load(self._h, block._b, packed.ctypes.data, packed.shape[1], packed.shape[0]))

    def scan_block(self, block: "Block", out_ptr: int, valid_ptr: int):
        """Scan of a loaded block into device buffers (asynchronous; sync() before reading)."""
        check(self._L.sgx_scan_block(self._h, block._b, out_ptr, valid_ptr))

    def synth_2bit_dev(self, packed_ptr: int, bpv: int, m: int, first_variant: int, seed: int,
                       thr_ptr: int):
        check(self._L.sgx_synth_2bit_dev(self._h, packed_ptr, bpv, self.n, m, first_variant, seed,
                                         thr_ptr))

    def sync(self):
        check(self._L.sgx_sync(self._h))

    def stats(self) -> dict:
        st = SgxStats()
        check(self._L.sgx_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def stats_total(self, reset: bool = True):
        """Sums over the calls completed since the last reset -> (dict, n_calls); syncs."""
        st, n = SgxStats(), C.c_uint64(0)
        check(self._L.sgx_get_stats_total(self._h, C.byref(st), C.byref(n), 1 if reset else 0))
        return st.as_dict(), int(n.value)

    def set_option(self, name: str, value: int):
        check(self._L.sgx_set_option(self._h, name.encode(), int(value)))

    def score_layout(self):
        """(limb counts of the score columns c'(K), e(K), s, w; number of column groups, 0 = FP64 path)."""
        p = 2 * self.k + 2
        limbs = np.zeros(p, dtype=np.int32)
        ng = C.c_int32(0)
        check(self._L.sgx_score_layout(self._h, limbs.ctypes.data, p, C.byref(ng)))
        return limbs, int(ng.value)

    def set_thresholds(self, maf, mac, missing, spa_pval):
        check(self._L.sgx_set_thresholds(self._h, maf, mac, missing, spa_pval))


class Block(_Handle):
    """A block of variants resident on the device (``sgx_block``: the 2-bit rows, the positions of their missing
    genotypes, the carrier lists of the rare variants): depends on the number of samples only, so one loaded
    block can be scanned with any number of models.  ``clist_avg`` (test hook): room of the carrier lists in
    entries per variant."""

    _attr, _free = "_b", "sgx_block_free"

    def __init__(self, n_samp: int, max_variants: int, device: int = 0, clist_avg: int = None):
        b = C.c_void_p()
        if clist_avg is None:
            check(self._L.sgx_block_create(int(n_samp), int(max_variants), int(device), C.byref(b)))
        else:
            check(self._L.sgx_block_create_ex(int(n_samp), int(max_variants), int(device), int(clist_avg), C.byref(b)))
        self._b = b
        self.n, self.cap = int(n_samp), int(max_variants)

    def load_dbit2(self, sc: "Scanner", alleles, bit0: int, n_file_samp: int, n_rows=None, sel=None, n_variants: int = None):
        """``genotype/data`` rows as the file stores them -> block, decoded on the device (``sgx_block_load_dbit2``;
        arguments as ``Scanner.scan_dbit2``): the block ``Scanner.load_block`` makes of the host-decoded rows."""
        a, n_rows, sel, m = _dbit2_args(alleles, bit0, n_file_samp, n_rows, sel, self.n, n_variants)
        check(self._L.sgx_block_load_dbit2(sc._h, self._b, a.ctypes.data, int(bit0), int(n_file_samp),
                                           None if n_rows is None else n_rows.ctypes.data,
                                           None if sel is None else sel.ctypes.data, m))

    @staticmethod
    def nbytes(n_samp: int, max_variants: int) -> int:
        return int(load().sgx_block_bytes(int(n_samp), int(max_variants)))

    @property
    def n_variants(self) -> int:
        return int(self._L.sgx_block_variants(self._b))


class DosageBlock(_Handle):
    """A batch of dosage rows resident on the device (``sgx_dsblock``) for the aggregate tests: loaded once, it
    serves the per-variant counts, the single-variant test of every row, the burden rows of all units and the SKAT
    sums of all units.
    ``dtype``: uint8 (0xFF = missing), int32 (INT_MIN = missing) or float64 (NaN / Inf = missing)."""

    _attr, _free = "_b", "sgx_dsblock_free"

    def __init__(self, sc: Scanner, dtype, max_variants: int):
        dt = np.dtype(dtype)
        if dt not in DS_DTYPES:
            raise TypeError("the dosages should be uint8, int32 or float64")
        self.dtype, self._sc = dt, sc
        self.n, self.cap, self.n_variants = sc.n, int(max_variants), 0
        b = C.c_void_p()
        check(self._L.sgx_dsblock_create(sc.n, DS_DTYPES[dt], self.cap, int(sc.device), C.byref(b)))
        self._b = b

    def load(self, dosage: np.ndarray):
        """Rows [m, N] in host memory -> block; returns (n_valid int32, sum float64, sum_trunc int64) per variant."""
        dosage = np.ascontiguousarray(dosage, dtype=self.dtype)
        if dosage.ndim != 2 or dosage.shape[1] != self.n:
            raise ValueError(f"Invalid length of dosages: {dosage.shape[-1]}.")
        m = dosage.shape[0]
        nv, sm, st = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float64), np.empty(m, dtype=np.int64)
        check(self._L.sgx_dsblock_load(self._sc._h, self._b, dosage.ctypes.data, m, nv.ctypes.data, sm.ctypes.data,
                                       st.ctypes.data))
        self.n_variants = m
        return nv, sm, st

    def load_packed(self, raw: np.ndarray, cls, scale: float, offset: float, sel=None):
        """Packed-real rows as the file stores them -> a float64 block, decoded and sample-selected on the device
        (``sgx_ds_block_load_packed``; arguments as ``Scanner.scan_packed``); returns what ``load`` of the decoded
        rows returns."""
        raw, code, sel = _packed_args(raw, cls, self.n, sel)
        m = raw.shape[0]
        nv, sm, st = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float64), np.empty(m, dtype=np.int64)
        check(self._L.sgx_ds_block_load_packed(self._sc._h, self._b, raw.ctypes.data, code, raw.shape[1], float(scale),
                                              float(offset), None if sel is None else sel.ctypes.data, m,
                                              nv.ctypes.data, sm.ctypes.data, st.ctypes.data))
        self.n_variants = m
        return nv, sm, st

    def scan(self):
        """Single-variant test of every resident row -> (out [m, 8], valid [m])."""
        out, valid = self._sc._out(self.n_variants)
        check(self._L.sgx_dsblock_scan(self._sc._h, self._b, out.ctypes.data, valid.ctypes.data))
        return out, valid

    def burden(self, grp_ptr, var_idx, flip, w, mw):
        """Burden rows of the groups (CSR over the block's rows) x the columns of ``w`` / ``mw`` ([entries, n_cols],
        NaN weight = entry not in that column), then the single-variant test -> (out [groups * n_cols, 8], valid)."""
        var_idx = np.ascontiguousarray(var_idx, dtype=np.int32)
        flip = np.ascontiguousarray(flip, dtype=np.uint8)
        w = np.ascontiguousarray(w, dtype=np.float64)
        mw = np.ascontiguousarray(mw, dtype=np.float64)
        grp_ptr, ng = _csr_ptr("DosageBlock.burden", "inconsistent group / weight shapes", grp_ptr, var_idx,
                               [(w, w.shape[1:]), (mw, w.shape[1:])], w.ndim == 2 and flip.shape == var_idx.shape)
        nc = w.shape[1]
        out, valid = self._sc._out(ng * nc)
        check(self._L.sgx_dsblock_burden(self._sc._h, self._b, ng, grp_ptr.ctypes.data, var_idx.ctypes.data,
                                         flip.ctypes.data, nc, w.ctypes.data, mw.ctypes.data, out.ctypes.data,
                                         valid.ctypes.data))
        return out, valid

    def collapse(self, grp_ptr, var_idx, flip, return_rows: bool = False):
        """One pseudo-variant per group of resident rows (CSR ``grp_ptr`` / ``var_idx`` over the block's rows, one flip
        byte per entry; ``sgx_ds_block_collapse``): per sample the largest minor-allele dosage over the
        group's entries (2 - x where ``flip``, 0 where missing), appended to the block as rows ``n_variants ..`` in the
        block's resident form -> (n_valid, sum, sum_trunc: what ``load`` returns for them; out [groups, 8], valid: what
        ``scan`` returns for them[; rows [groups, N]: uint8 for a uint8 block, else float64])."""
        flip = np.ascontiguousarray(flip, dtype=np.uint8)
        grp_ptr, var_idx, ng, _, _ = _unit_args("DosageBlock.collapse", grp_ptr, var_idx, [(flip, ())])
        nv, sm, st = np.empty(ng, dtype=np.int32), np.empty(ng, dtype=np.float64), np.empty(ng, dtype=np.int64)
        out, valid = self._sc._out(ng)
        rows = np.empty((ng, self.n), dtype=np.uint8 if self.dtype == np.uint8 else np.float64) if return_rows else None
        check(self._L.sgx_ds_block_collapse(self._sc._h, self._b, ng, grp_ptr.ctypes.data, var_idx.ctypes.data,
                                            flip.ctypes.data, nv.ctypes.data, sm.ctypes.data, st.ctypes.data,
                                            out.ctypes.data, valid.ctypes.data, None if rows is None else rows.ctypes.data))
        self.n_variants += ng
        return (nv, sm, st, out, valid, rows) if return_rows else (nv, sm, st, out, valid)

    def skat(self, unit_ptr, var_idx, flip, mean):
        """Score statistics and their covariance per unit (CSR over the block's rows; per entry ``flip`` and the mean
        that stands in for a missing dosage, already flipped; ``sgx_ds_block_skat``) -> (score [entries], cov: per unit
        an [m, m] symmetric matrix), as ``Scanner.skat_2bit``."""
        flip = np.ascontiguousarray(flip, dtype=np.uint8)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        unit_ptr, var_idx, n_units, sizes, offs = _unit_args("DosageBlock.skat", unit_ptr, var_idx, [(flip, ()), (mean, ())])
        score, cov = np.zeros(max(1, var_idx.size)), np.zeros(max(1, int(offs[-1])))
        if var_idx.size:
            check(self._L.sgx_ds_block_skat(self._sc._h, self._b, n_units, unit_ptr.ctypes.data, var_idx.ctypes.data,
                                            flip.ctypes.data, mean.ctypes.data, score.ctypes.data, cov.ctypes.data))
        return score[:var_idx.size], _unit_matrices(cov, sizes, offs)

    def cond_set(self, var_idx, flip, mean):
        """Installs the conditioning set of the conditional scan from resident rows (``sgx_ds_block_cond_set``): 0 to
        ``COND_MAX`` rows ``var_idx`` with ``flip`` / ``mean`` as for ``skat`` -> (S_C [C], Phi_CC [C, C]), equal to
        ``skat`` on them as one unit bit for bit.  The scanner keeps the set (as ``Scanner.cond_set`` does) beyond the
        block's next load; no row clears it."""
        flip, mean, var_idx = _flip_mean("DosageBlock.cond_set", "inconsistent table shapes", flip, mean, var_idx)
        c = var_idx.size
        score, cov = np.zeros(max(1, c)), np.zeros(max(1, c * c))
        check(self._L.sgx_ds_block_cond_set(self._sc._h, self._b, c, var_idx.ctypes.data, flip.ctypes.data,
                                            mean.ctypes.data, score.ctypes.data, cov.ctypes.data))
        self._sc._n_cond = c
        return score[:c], cov[:c * c].reshape(c, c)

    def cond(self, flip, mean):
        """Score, variance and covariances with the installed set of every resident row (``flip`` / ``mean`` per
        resident row; ``sgx_ds_block_cond``) -> (score [m], var [m], cov [m, C])."""
        m = self.n_variants
        flip, mean, _ = _flip_mean("DosageBlock.cond", "one flip and one mean per resident row", flip, mean, n=m)
        c = int(getattr(self._sc, "_n_cond", 0))
        score, var, cov = np.zeros(max(1, m)), np.zeros(max(1, m)), np.zeros(max(1, m * c))
        check(self._L.sgx_ds_block_cond(self._sc._h, self._b, flip.ctypes.data, mean.ctypes.data, score.ctypes.data,
                                        var.ctypes.data, cov.ctypes.data))
        return score[:m], var[:m], cov[:m * c].reshape(m, c)

    def firth(self, var_idx, flip, mean, maxit: int = 50):
        """Firth bias-reduced effect size of the resident rows ``var_idx`` (any order, repeats allowed) with ``flip`` /
        ``mean`` per entry as for ``skat`` (``sgx_ds_block_firth``; binary traits) -> out4 [n_rows, 4]: beta for the
        entry's orientation, SE, iterations, converged (1 / 0), as ``Scanner.firth_2bit`` -- bit for bit what it gives on
        the 2-bit form of a row of hard calls.  NaN / NaN / 0 for a row without a non-zero dosage or with a non-finite
        mean."""
        flip, mean, var_idx = _flip_mean("DosageBlock.firth", "one flip and one mean per entry of var_idx", flip, mean, var_idx)
        m = var_idx.size
        out4 = np.zeros((max(1, m), 4))
        check(self._L.sgx_ds_block_firth(self._sc._h, self._b, m, var_idx.ctypes.data, flip.ctypes.data, mean.ctypes.data,
                                         int(maxit), out4.ctypes.data))
        return out4[:m]

    def skat_kmat(self, op, unit_ptr, var_idx, flip, mean, w, tau, maxiter: int = 500, tol: float = 1e-5):
        """``skat`` with the covariance under the fitted model on the explicit GRM of ``op`` (an ``ExplicitGrmOperator``
        on the scanner's device), ``Phi^K = A' P A`` as ``Scanner.skat_kmat`` defines it (``sgx_ds_block_skat_kmat``) ->
        (score [entries], cov: per unit an [m, m] symmetric matrix, iters [entries]: PCG steps of every entry's solve).
        An entry whose mean is not finite gets non-finite results, whether or not a sample of its row is missing."""
        flip = np.ascontiguousarray(flip, dtype=np.uint8)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        w, tau = _sigma_args("DosageBlock.skat_kmat", op, w, tau)
        unit_ptr, var_idx, n_units, sizes, offs = _unit_args("DosageBlock.skat_kmat", unit_ptr, var_idx,
                                                             [(flip, ()), (mean, ())])
        score, cov = np.zeros(max(1, var_idx.size)), np.zeros(max(1, int(offs[-1])))
        iters = np.zeros(max(1, var_idx.size), dtype=np.int32)
        if var_idx.size:
            check(self._L.sgx_ds_block_skat_kmat(self._sc._h, op._h, self._b, n_units, unit_ptr.ctypes.data,
                                                 var_idx.ctypes.data, flip.ctypes.data, mean.ctypes.data, w.ctypes.data,
                                                 tau.ctypes.data, int(maxiter), float(tol), score.ctypes.data,
                                                 cov.ctypes.data, iters.ctypes.data))
        return score[:var_idx.size], _unit_matrices(cov, sizes, offs), iters[:var_idx.size]

    def cond_kmat_set(self, op, var_idx, flip, mean, w, tau, maxiter: int = 500, tol: float = 1e-5):
        """Installs the conditioning set of the conditional scan on the explicit GRM of ``op`` from resident rows
        (``sgx_ds_block_cond_kmat_set``): rows ``var_idx`` with ``flip`` / ``mean`` as for ``skat`` -> (S_C [C],
        Phi^K_CC [C, C], iters [C]), equal to ``skat_kmat`` on them as one unit bit for bit.  The scanner keeps the set
        (the one ``Scanner.cond_kmat_set`` fills) beyond the block's next load; no row clears it."""
        flip, mean, var_idx = _flip_mean("DosageBlock.cond_kmat_set", "inconsistent table shapes", flip, mean, var_idx)
        w, tau = _sigma_args("DosageBlock.cond_kmat_set", op, w, tau)
        c = var_idx.size
        score, cov, iters = np.zeros(max(1, c)), np.zeros(max(1, c * c)), np.zeros(max(1, c), dtype=np.int32)
        check(self._L.sgx_ds_block_cond_kmat_set(self._sc._h, op._h, self._b, c, var_idx.ctypes.data, flip.ctypes.data,
                                                 mean.ctypes.data, w.ctypes.data, tau.ctypes.data, int(maxiter),
                                                 float(tol), score.ctypes.data, cov.ctypes.data, iters.ctypes.data))
        self._sc._n_cond_kmat = c
        return score[:c], cov[:c * c].reshape(c, c), iters[:c]

    def cond_kmat(self, op, flip, mean):
        """Score, variance and covariances with the set of ``cond_kmat_set`` of every resident row under the fitted model
        on the explicit GRM (``flip`` / ``mean`` per resident row; ``sgx_ds_block_cond_kmat``) -> (score [m], var [m],
        cov [m, C], iters [m]: PCG steps of the row's column), as ``Scanner.cond_kmat``."""
        m = self.n_variants
        flip, mean, _ = _flip_mean("DosageBlock.cond_kmat", "one flip and one mean per resident row", flip, mean, n=m)
        c = int(getattr(self._sc, "_n_cond_kmat", 0))
        score, var, cov = np.zeros(max(1, m)), np.zeros(max(1, m)), np.zeros(max(1, m * c))
        iters = np.zeros(max(1, m), dtype=np.int32)
        check(self._L.sgx_ds_block_cond_kmat(self._sc._h, op._h, self._b, flip.ctypes.data, mean.ctypes.data,
                                             score.ctypes.data, var.ctypes.data, cov.ctypes.data, iters.ctypes.data))
        return score[:m], var[:m], cov[:m * c].reshape(m, c), iters[:m]


class PinnedBuffer:
    """Page-locked host memory (``sgx_host_alloc``) as a numpy array: block buffers filled by the GDS
    decoder and handed to the host-buffer scans cross PCIe at the full link rate."""

    def __init__(self, shape, dtype=np.uint8):
        self._L = load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = self._L.sgx_host_alloc(max(1, self.nbytes))
        if not self._p:
            raise MemoryError(self._L.sgx_last_error().decode())
        buf = (C.c_uint8 * max(1, self.nbytes)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            self._L.sgx_host_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def decode_dbit2(alleles, bit0: int, n_samp: int, m: int, out: np.ndarray, sel: np.ndarray = None, threads: int = 0):
    """SeqArray allele codes (bytes of genotype/data from bit ``bit0`` on) -> 2-bit dosage rows in ``out``
    ([>= m, >= ceil(n / 4)] uint8, C-contiguous rows); ``sgx_decode_dbit2``, host threads, no GPU needed."""
    L = load()
    a = np.frombuffer(alleles, dtype=np.uint8) if not isinstance(alleles, np.ndarray) else alleles
    if out.dtype != np.uint8 or out.ndim != 2 or out.strides[1] != 1 or out.shape[0] < m:
        raise ValueError("decode_dbit2: out must be a [>= m, stride] uint8 array with contiguous rows")
    if out.strides[0] != out.shape[1]:
        # (the library zeroes a row's bytes from the last code up to its stride: a column slice of a wider buffer
        # would have the neighbouring columns cleared, and the last row would be written past the allocation)
        raise ValueError("decode_dbit2: out must own whole rows (a column slice of a wider buffer is not accepted)")
    need = (bit0 + m * n_samp * 4 + 7) // 8
    if a.size < need:
        raise ValueError("decode_dbit2: allele buffer too short")
    sp, ns = None, 0
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.int64)
        sp, ns = sel.ctypes.data, int(sel.size)
    check(L.sgx_decode_dbit2(a.ctypes.data, int(bit0), int(n_samp), int(m), sp, ns, out.ctypes.data, int(out.strides[0]), int(threads)))
    return out


def geno_stats_2bit(packed: np.ndarray, n_samp: int, device: int = 0):
    """Per-variant (n_valid, allele_sum) of a host 2-bit matrix, counted on the GPU."""
    L = load()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    m = packed.shape[0]
    nv, sm = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
    check(L.sgx_geno_stats_2bit(packed.ctypes.data, packed.shape[1], int(n_samp), m, int(device),
                                nv.ctypes.data, sm.ctypes.data))
    return nv, sm


class LdEngine(_Handle):
    """The LD handle of the library (``sgx_ld``) for rows of ``n_samp`` samples at ``bytes_per_variant``
    stride: a resident block of up to ``LD_BLOCK`` candidate rows and a window of kept rows (a ring of at most
    ``window_bytes``; 0: the library's default).  What seqFitLDpruning drives; needs no model."""

    _free = "sgx_ld_free"

    def __init__(self, n_samp: int, bytes_per_variant: int, device: int = 0, window_bytes: int = 0):
        self.n_samp, self.bpv = int(n_samp), int(bytes_per_variant)
        h = C.c_void_p()
        check(self._L.sgx_ld_create(int(device), self.n_samp, self.bpv, int(window_bytes), C.byref(h)))
        self._h = h

    def _rows(self, rows) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        if rows.ndim != 2 or rows.shape[1] != self.bpv:
            raise ValueError(f"LdEngine: rows must be [m, {self.bpv}] uint8")
        return rows

    def counts(self, a, b) -> np.ndarray:
        """int32 [ma, mb, 6] = (n, sx, sy, sxx, syy, sxy) of every pair (row of ``a``: x, row of ``b``: y)."""
        a, b = self._rows(a), self._rows(b)
        out = np.zeros((a.shape[0], b.shape[0], 6), dtype=np.int32)
        check(self._L.sgx_ld_counts_2bit(self._h, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], out.ctypes.data))
        return out

    def block(self, rows, t2: float) -> np.ndarray:
        """Uploads the candidate rows -> uint8 [mb, W + mb], 1 = in LD at ``t2``: the W window rows oldest first, then
        the block's own rows (only j < i defined)."""
        rows = self._rows(rows)
        flags = np.zeros((rows.shape[0], self.window_len + rows.shape[0]), dtype=np.uint8)
        check(self._L.sgx_ld_block_2bit(self._h, rows.ctypes.data, rows.shape[0], float(t2), flags.ctypes.data))
        return flags

    def push(self, keep_idx, drop_oldest: int = 0):
        """Drops the oldest ``drop_oldest`` window rows, then appends the block's rows ``keep_idx`` (ascending).  A
        window over the byte budget raises MemoryError."""
        idx = np.ascontiguousarray(keep_idx, dtype=np.int32).reshape(-1)
        rc = self._L.sgx_ld_window_push(self._h, idx.ctypes.data if idx.size else None, idx.size, int(drop_oldest))
        if rc == -3:                                   # SGX_ENOMEM
            raise MemoryError(self._L.sgx_last_error().decode("utf-8", "replace"))
        check(rc)

    def reset(self):
        check(self._L.sgx_ld_window_reset(self._h))

    @property
    def window_len(self) -> int:
        return int(self._L.sgx_ld_window_len(self._h))

    def kernel_ms(self) -> float:
        ms = C.c_double()
        check(self._L.sgx_ld_kernel_ms(self._h, C.byref(ms)))
        return ms.value


def ld_counts_2bit(packed_a, packed_b, n_samp: int, device: int = 0) -> np.ndarray:
    """The six LD sums of every pair of 2-bit rows, on the GPU: int32 [ma, mb, 6] = (n, sx, sy, sxx, syy, sxy) over the
    samples called in both rows (``sgx_ld_counts_2bit``); the two matrices share their row stride."""
    a = np.ascontiguousarray(packed_a, dtype=np.uint8)
    b = np.ascontiguousarray(packed_b, dtype=np.uint8)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("ld_counts_2bit: two [m, stride] uint8 matrices of one stride")
    out = np.zeros((a.shape[0], b.shape[0], 6), dtype=np.int32)
    with LdEngine(n_samp, a.shape[1], device=device) as eng:
        for i in range(0, a.shape[0], LD_MAX_ROWS):
            for j in range(0, b.shape[0], LD_MAX_ROWS):
                out[i:i + LD_MAX_ROWS, j:j + LD_MAX_ROWS] = eng.counts(a[i:i + LD_MAX_ROWS], b[j:j + LD_MAX_ROWS])
    return out


def ld_corr(counts) -> np.ndarray:
    """The six sums [..., 6] -> r = c / sqrt(vx vy) with c = n sxy - sx sy, vx = n sxx - sx^2, vy = n syy - sy^2 in
    int64; NaN where vx vy == 0.  numpy, no GPU."""
    s = np.asarray(counts).astype(np.int64)
    n, sx, sy, sxx, syy, sxy = (s[..., k] for k in range(6))
    c, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    den = np.sqrt(vx.astype(np.float64) * vy.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, c.astype(np.float64) / den, np.nan)


def king_values(counts):
    """KING-robust kinship and IBS0 from the five counts [5, ...] (nn, hi, hj, hh, ibs0), the expressions of
    ``sgx_grm_king_pairs`` in numpy float64 (the same bits): D = (hi + hj - 2 hh) + 4 ibs0, mn = min(hi, hj),
    kinship = 0.5 - D / (4 mn) (NaN where mn == 0), IBS0 = ibs0 / nn (NaN where nn == 0)."""
    c = np.asarray(counts).astype(np.int64)
    nn, hi, hj, hh, ibs0 = (c[k] for k in range(5))
    D, mn = (hi + hj - 2 * hh) + 4 * ibs0, np.minimum(hi, hj)
    with np.errstate(invalid="ignore", divide="ignore"):
        kin = np.where(mn > 0, 0.5 - D.astype(np.float64) / (4.0 * mn.astype(np.float64)), np.nan)
        ibs = np.where(nn > 0, ibs0.astype(np.float64) / nn.astype(np.float64), np.nan)
    return kin, ibs


def quantize_packed(raw, cls, scale, offset, n_samp: int, sel=None, device: int = 0, chunk_bytes: int = 0):
    """Stored dosage rows -> the 2-bit hard-call rows of the null-model fit and the marker filter's counts, on the GPU
    (``sgx_quantize_packed``): ``raw`` [m, n_file_samp] of class ``cls`` as for ``Scanner.scan_packed``, ``sel``: the
    ``n_samp`` samples wanted as indices into the file's, or None (all, in the file's order).  Returns (packed
    [m, ceil(n_samp / 4)], n_valid, allele_sum, ds_valid, ds_sum): what ``gds.quantize_dosage_2bit`` states in numpy."""
    L = load()
    n_samp = int(n_samp)
    raw, code, sel = _packed_args(raw, cls, n_samp, sel)
    m = raw.shape[0]
    packed = np.zeros((m, (max(n_samp, 0) + 3) // 4), dtype=np.uint8)
    nv, sm, dv = (np.zeros(m, dtype=np.int32) for _ in range(3))
    dsum = np.zeros(m, dtype=np.float64)
    check(L.sgx_quantize_packed(raw.ctypes.data, code, raw.shape[1], float(scale), float(offset),
                                None if sel is None else sel.ctypes.data, n_samp, m, int(device), int(chunk_bytes),
                                packed.ctypes.data, packed.shape[1], nv.ctypes.data, sm.ctypes.data, dv.ctypes.data,
                                dsum.ctypes.data))
    return packed, nv, sm, dv, dsum


class _Operator(_Handle):
    """What the operators on a GRM of ``n`` samples share: the entry points that the library has once per kind of
    GRM under the same name and prototype, ``_prefix`` + name.  Several right-hand sides are the rows of B ([k, N]),
    k of any size: they go to the library in batches of GRM_MAX_RHS."""

    _prefix = None

    def _fn(self, name: str):
        return getattr(self._L, self._prefix + name)

    def _rhs(self, B) -> np.ndarray:
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[1] != self.n:
            raise ValueError("B must be [k, N]: one right-hand side of N samples per row")
        return B

    def _weights(self, w) -> np.ndarray:
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (self.n,):
            raise ValueError("w must have one entry per sample")
        return w

    @staticmethod
    def _batches(k: int):
        return [(j0, min(GRM_MAX_RHS, k - j0)) for j0 in range(0, k, GRM_MAX_RHS)]

    def sync(self):
        check(self._fn("sync")(self._h))

    def diag(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        check(self._fn("diag")(self._h, out.ctypes.data))
        return out

    def crossprod_many(self, B: np.ndarray) -> np.ndarray:
        """GRM b_j for every row b_j of B ([k, N] -> [k, N]); row j equals crossprod(B[j]) bit for bit."""
        B = self._rhs(B)
        out = np.empty_like(B)
        for j0, k in self._batches(B.shape[0]):
            check(self._fn("crossprod_multi")(self._h, B[j0].ctypes.data, self.n, k, out[j0].ctypes.data))
        return out

    def crossprod_many_dev(self, b_ptr: int, ldb: int, k: int, out_ptr: int):
        """Device form: k vectors at b_ptr + j * ldb doubles (asynchronous until sync())."""
        check(self._fn("crossprod_multi_dev")(self._h, b_ptr, int(ldb), int(k), out_ptr))

    def pcg_many(self, w: np.ndarray, tau, B: np.ndarray, maxiter: int = 500, tol: float = 1e-5):
        """pcg on every row of B in lockstep -> (X [k, N], iters [k]); row j equals pcg(w, tau, B[j])
        bit for bit, with the same iteration count."""
        B, w = self._rhs(B), self._weights(w)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        X = np.empty_like(B)
        iters = np.zeros(B.shape[0], dtype=np.int32)
        for j0, k in self._batches(B.shape[0]):
            check(self._fn("pcg_multi")(self._h, w.ctypes.data, tau.ctypes.data, B[j0].ctypes.data, self.n, k,
                                        int(maxiter), float(tol), X[j0].ctypes.data, iters[j0:].ctypes.data))
        return X, iters


class GrmOperator(_Operator):
    """Implicit GRM of the null-model fit on one GPU (``sgx_grm``): the operator
    behind ``saige_store_2b_geno`` / ``get_crossprod_b_grm`` / ``PCG_diag_sigma``
    (reference src/saige_fitnull.cpp:159-230, 435-536, 581-614)."""

    _prefix, _free = "sgx_grm_", "sgx_grm_free"

    def __init__(self, packed, n_samp: int, device: int = 0, dev_ptr: int = 0, n_markers: int = 0,
                 bytes_per_marker: int = 0):
        """packed: numpy [n_markers, bytes_per_marker]; or dev_ptr/n_markers/bytes_per_marker
        for a matrix already in this GPU's memory."""
        L = load()
        h = C.c_void_p()
        self.n = int(n_samp)
        if dev_ptr:
            self.m = int(n_markers)
            check(L.sgx_grm_init_dev(dev_ptr, int(bytes_per_marker), self.n, self.m, int(device), C.byref(h)))
        else:
            packed = np.ascontiguousarray(packed, dtype=np.uint8)
            if packed.ndim != 2:
                raise ValueError("packed genotypes must be [n_markers, bytes_per_marker]")
            self.m = int(packed.shape[0])
            check(L.sgx_grm_init(packed.ctypes.data, packed.shape[1], self.n, self.m, int(device), C.byref(h)))
        self._h = h

    def crossprod_dev(self, b_ptr: int, out_ptr: int):
        check(self._L.sgx_grm_crossprod_dev(self._h, b_ptr, out_ptr))

    # -- the explicit GRM (sgx_grm_dense / sgx_grm_sparse); marker groups are ignored
    DENSE_BLOCK = 4096     # rows / columns per sgx_grm_dense call of dense()

    def dense_block(self, i0: int, ni: int, j0: int, nj: int) -> np.ndarray:
        """K[i0:i0+ni, j0:j0+nj] of the GRM K = G'G/M, [ni, nj] float64."""
        out = np.empty((max(int(ni), 0), max(int(nj), 0)), dtype=np.float64)
        check(self._L.sgx_grm_dense(self._h, int(i0), int(ni), int(j0), int(nj), out.ctypes.data, out.shape[1]))
        return out

    def dense_kernel_ms(self) -> float:
        """Device milliseconds of the kernels of the last dense_block call (without the copy to the host)."""
        ms = C.c_double(0)
        check(self._L.sgx_grm_dense_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def dense(self) -> np.ndarray:
        """The whole GRM [N, N]: the blocks on and above the diagonal, the others mirrored."""
        n, bs = self.n, self.DENSE_BLOCK
        K = np.empty((n, n), dtype=np.float64)
        for i0 in range(0, n, bs):
            ni = min(bs, n - i0)
            for j0 in range(i0, n, bs):
                nj = min(bs, n - j0)
                blk = self.dense_block(i0, ni, j0, nj)
                K[i0:i0 + ni, j0:j0 + nj] = blk
                if j0 != i0:
                    K[j0:j0 + nj, i0:i0 + ni] = blk.T
        return K

    def sparse(self, cutoff: float, cap: Optional[int] = None, return_stats: bool = False):
        """The pairs i <= j with K_ij >= cutoff and every diagonal entry -> (i, j, x), sorted by (i, j); x holds
        the numbers dense() gives.  Retries once with the size the library reports when ``cap`` entries (default
        8 N) do not hold them.  With ``return_stats`` the dict of sgx_grm_sparse_stats comes fourth."""
        cap = int(8 * self.n if cap is None else cap)
        for attempt in (0, 1):
            i = np.empty(cap, dtype=np.int32)
            j = np.empty(cap, dtype=np.int32)
            x = np.empty(cap, dtype=np.float64)
            n_out = C.c_size_t(0)
            st = SgxGrmSparseStats()
            rc = self._L.sgx_grm_sparse(self._h, float(cutoff), cap, i.ctypes.data, j.ctypes.data, x.ctypes.data,
                                        C.byref(n_out), C.byref(st))
            if rc == ENOSPACE and attempt == 0:
                cap = int(n_out.value)
                continue
            check(rc)
            k = int(n_out.value)
            res = (i[:k].copy(), j[:k].copy(), x[:k].copy())
            return res + (st.as_dict(),) if return_stats else res

    # -- KING-robust kinship (sgx_grm_king_counts / sgx_grm_king_pairs); marker groups are ignored
    def king_counts(self, i0: int, ni: int, j0: int, nj: int) -> np.ndarray:
        """The five counts (nn, hi, hj, hh, ibs0) of the pairs [i0, i0 + ni) x [j0, j0 + nj): int32 [5, ni, nj], over
        the markers where both samples are called (``king_values`` turns them into kinship and IBS0)."""
        out = np.empty((5, max(int(ni), 0), max(int(nj), 0)), dtype=np.int32)
        check(self._L.sgx_grm_king_counts(self._h, int(i0), int(ni), int(j0), int(nj), out.ctypes.data, out.shape[2]))
        return out

    def king_pairs(self, cutoff: float, cap: Optional[int] = None, return_stats: bool = False):
        """The pairs i < j with KING-robust kinship >= cutoff -> (i, j, kinship, ibs0, counts [pairs, 5]), sorted by
        (i, j); the numbers are those of ``king_values(king_counts(...))``.  Retries once with the size the library
        reports when ``cap`` pairs (default 8 N) do not hold them.  With ``return_stats`` the dict of
        sgx_grm_king_stats comes sixth."""
        cap = int(8 * self.n if cap is None else cap)
        for attempt in (0, 1):
            i = np.empty(cap, dtype=np.int32)
            j = np.empty(cap, dtype=np.int32)
            kin = np.empty(cap, dtype=np.float64)
            ibs = np.empty(cap, dtype=np.float64)
            cnt = np.empty((cap, 5), dtype=np.int32)
            n_out = C.c_size_t(0)
            st = SgxGrmKingStats()
            rc = self._L.sgx_grm_king_pairs(self._h, float(cutoff), cap, i.ctypes.data, j.ctypes.data, kin.ctypes.data,
                                            ibs.ctypes.data, cnt.ctypes.data, C.byref(n_out), C.byref(st))
            if rc == ENOSPACE and attempt == 0:
                cap = int(n_out.value)
                continue
            check(rc)
            k = int(n_out.value)
            res = (i[:k].copy(), j[:k].copy(), kin[:k].copy(), ibs[:k].copy(), cnt[:k].copy())
            return res + (st.as_dict(),) if return_stats else res

    # -- the marker side of the product and the principal components of K (sgx_grm_marker_dots / sgx_grm_pca)
    def marker_table(self):
        """(af, inv) per marker: the allele frequency and 1 / sqrt(2 af (1 - af)) the operator standardises with."""
        af, inv = np.empty(self.m, dtype=np.float64), np.empty(self.m, dtype=np.float64)
        check(self._L.sgx_grm_marker_table(self._h, af.ctypes.data, inv.ctypes.data))
        return af, inv

    def marker_dots(self, B: np.ndarray) -> np.ndarray:
        """dot_v = sum_i G[v, i] b_i for every row b of B ([k, N] -> [k, M]): pass 1 of the product, as an output."""
        B = self._rhs(B)
        out = np.empty((B.shape[0], self.m), dtype=np.float64)
        for j0, k in self._batches(B.shape[0]):
            check(self._L.sgx_grm_marker_dots(self._h, B[j0].ctypes.data, self.n, k, out[j0].ctypes.data, self.m))
        return out

    def pca(self, n_pc: int, Q0: np.ndarray, max_iter: int = 100, tol: float = 1e-6, loadings: bool = False) -> dict:
        """The top ``n_pc`` eigenpairs of K by block subspace iteration from the rows of ``Q0`` ([n_block, N]) ->
        dict of ``eigval`` [n_pc], ``resid`` [n_pc] (|K u - theta u|), ``vec`` [n_pc, N], ``loading`` ([n_pc, M], or
        None), ``iters``, ``n_converged``, ``ms_products``, ``ms_block``.  A block that loses rank raises
        ``SgxRankError`` (a ValueError); not converging within ``max_iter`` is for the caller to read off ``resid``."""
        Q0 = self._rhs(Q0)
        n_pc, L = int(n_pc), Q0.shape[0]
        k = max(n_pc, 1)
        eigval, resid = np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
        vec = np.zeros((k, self.n), dtype=np.float64)
        load_ = np.zeros((k, self.m), dtype=np.float64) if loadings else None
        st = SgxGrmPcaStats()
        rc = self._L.sgx_grm_pca(self._h, n_pc, L, Q0.ctypes.data, self.n, int(max_iter), float(tol), eigval.ctypes.data,
                                 resid.ctypes.data, vec.ctypes.data, self.n, None if load_ is None else load_.ctypes.data,
                                 self.m, C.byref(st))
        if rc == ERANK:
            raise SgxRankError(rc, self._L.sgx_last_error().decode("utf-8", "replace"))
        check(rc)
        return {"eigval": eigval, "resid": resid, "vec": vec, "loading": load_, "iters": int(st.iters),
                "n_converged": int(st.n_converged), "ms_products": float(st.ms_products), "ms_block": float(st.ms_block)}

    def ts_gram(self, A: np.ndarray, B: Optional[np.ndarray] = None, n: Optional[int] = None) -> np.ndarray:
        """C[a, b] = sum_{i < n} A[a, i] B[b, i] by the block Gram kernel (``sgx_grm_ts_gram``; for tests): A [La, ld],
        B [Lb, ld'] (None: A itself), n rows (default: the whole rows).  Entries beyond n are never read."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = A if B is None else np.ascontiguousarray(B, dtype=np.float64)
        if A.ndim != 2 or B.ndim != 2:
            raise ValueError("ts_gram: two [L, ld] arrays")
        n = int(min(A.shape[1], B.shape[1]) if n is None else n)
        out = np.empty((A.shape[0], B.shape[0]), dtype=np.float64)
        check(self._L.sgx_grm_ts_gram(self._h, n, A.ctypes.data, A.shape[1], A.shape[0], B.ctypes.data, B.shape[1],
                                      B.shape[0], out.ctypes.data))
        return out

    def ts_apply(self, A: np.ndarray, T: np.ndarray, n: Optional[int] = None, fill: float = 0.0) -> np.ndarray:
        """Out[c, i] = sum_a A[a, i] T[a, c] for i < n by the block kernel (``sgx_grm_ts_apply``; for tests): A [La, ld],
        T [La, Lc] -> [Lc, ld], whose entries beyond n keep ``fill``."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        T = np.ascontiguousarray(T, dtype=np.float64)
        if A.ndim != 2 or T.ndim != 2 or T.shape[0] != A.shape[0]:
            raise ValueError("ts_apply: A [La, ld] and T [La, Lc]")
        n = int(A.shape[1] if n is None else n)
        out = np.full((T.shape[1], A.shape[1]), fill, dtype=np.float64)
        check(self._L.sgx_grm_ts_apply(self._h, n, A.ctypes.data, A.shape[1], A.shape[0], T.ctypes.data, T.shape[1],
                                       out.ctypes.data, A.shape[1]))
        return out

    def crossprod(self, b: np.ndarray) -> np.ndarray:
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (self.n,):
            raise ValueError("b must have one entry per sample")
        out = np.empty(self.n, dtype=np.float64)
        check(self._L.sgx_grm_crossprod(self._h, b.ctypes.data, out.ctypes.data))
        return out

    def pcg(self, w: np.ndarray, tau, b: np.ndarray, maxiter: int = 500, tol: float = 1e-5):
        w = self._weights(w)
        b = np.ascontiguousarray(b, dtype=np.float64)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        x = np.empty(self.n, dtype=np.float64)
        it = C.c_int(0)
        check(self._L.sgx_grm_pcg(self._h, w.ctypes.data, tau.ctypes.data, b.ctypes.data, int(maxiter),
                                  float(tol), x.ctypes.data, C.byref(it)))
        return x, int(it.value)

    # -- marker groups; a column of a *_loco call leaves one group out (excl[j], -1: none)
    def set_groups(self, group, n_groups: Optional[int] = None):
        """One group id per marker (0 <= id < n_groups <= GRM_MAX_GROUPS, any order, groups may be empty);
        n_groups defaults to max(group) + 1."""
        g = np.ascontiguousarray(np.clip(np.asarray(group, dtype=np.int64), -1, np.iinfo(np.int32).max), dtype=np.int32)
        if g.shape != (self.m,):
            raise ValueError("group must have one entry per marker")
        if n_groups is None:
            n_groups = int(g.max()) + 1
        check(self._L.sgx_grm_set_groups(self._h, g.ctypes.data, int(n_groups)))
        self.n_groups = int(n_groups)

    def group_sizes(self) -> np.ndarray:
        out = np.zeros(GRM_MAX_GROUPS, dtype=np.int64)
        check(self._L.sgx_grm_group_sizes(self._h, out.ctypes.data))
        return out[:getattr(self, "n_groups", 0)].copy()

    def diag_loco(self, excl: int) -> np.ndarray:
        """diag of the GRM of the markers outside group excl (-1: diag())."""
        out = np.empty(self.n, dtype=np.float64)
        check(self._L.sgx_grm_diag_loco(self._h, int(excl), out.ctypes.data))
        return out

    def _excl(self, excl, k: int) -> np.ndarray:
        e = np.ascontiguousarray(np.clip(np.asarray(excl, dtype=np.int64), -2, np.iinfo(np.int32).max), dtype=np.int32)
        if e.shape != (k,):
            raise ValueError("excl must name one group (or -1) per row of B")
        return e

    def crossprod_loco(self, B: np.ndarray, excl) -> np.ndarray:
        """Row j: the GRM of the markers outside group excl[j] times B[j] ([k, N] -> [k, N]).  A row's result
        depends only on its own b and excl; with excl[j] = -1 it is crossprod(B[j]) bit for bit."""
        B = self._rhs(B)
        e = self._excl(excl, B.shape[0])
        out = np.empty_like(B)
        for j0, k in self._batches(B.shape[0]):
            check(self._L.sgx_grm_crossprod_loco(self._h, B[j0].ctypes.data, self.n, k, e[j0:].ctypes.data,
                                                 out[j0].ctypes.data))
        return out

    def pcg_loco(self, W: np.ndarray, w_idx, tau, B: np.ndarray, excl, maxiter: int = 500, tol: float = 1e-5):
        """pcg on every row of B in lockstep, row j with the weights W[w_idx[j]] ([n_w, N]) on the GRM of the
        markers outside group excl[j] -> (X [k, N], iters [k]).  A row's result depends only on its own b, w
        and excl; one w and excl = -1 give pcg_many's bits."""
        B = self._rhs(B)
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.n or W.shape[0] < 1:
            raise ValueError("W must be [n_w, N]: one weight vector of N samples per row")
        wi = np.asarray(w_idx, dtype=np.int64)
        if wi.shape != (B.shape[0],) or (wi.size and (wi.min() < 0 or wi.max() >= W.shape[0])):
            raise ValueError("w_idx must name one row of W per row of B")
        e = self._excl(excl, B.shape[0])
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        X = np.empty_like(B)
        iters = np.zeros(B.shape[0], dtype=np.int32)
        for j0, k in self._batches(B.shape[0]):
            rows, loc = np.unique(wi[j0:j0 + k], return_inverse=True)     # the weight rows this batch uses
            Wb = np.ascontiguousarray(W[rows])
            loc = np.ascontiguousarray(loc, dtype=np.int32)
            check(self._L.sgx_grm_pcg_loco(self._h, Wb.ctypes.data, self.n, int(rows.size), loc.ctypes.data,
                                           tau.ctypes.data, B[j0].ctypes.data, self.n, k, e[j0:].ctypes.data,
                                           int(maxiter), float(tol), X[j0].ctypes.data, iters[j0:].ctypes.data))
        return X, iters


def csr_of_upper(n: int, i, j, x):
    """The full symmetric CSR (row_ptr int64 [n + 1], col int32, val float64; columns ascending within a row) of
    a matrix given by its upper triangle (i <= j, each pair once)."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    off = i != j
    rows, cols = np.concatenate([i, j[off]]), np.concatenate([j, i[off]])
    vals = np.concatenate([x, x[off]])
    o = np.lexsort((cols, rows))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_ptr[1:])
    return row_ptr, np.ascontiguousarray(cols[o], dtype=np.int32), np.ascontiguousarray(vals[o])


class ExplicitGrmOperator(_Operator):
    """Operator of an explicit GRM resident on one GPU (``sgx_kmat``): what ``seqFitNullGLMM_SPA(grm_mat=)`` fits
    the null model on.  ``grm``: a ``SparseGRM`` (its upper triangle is expanded to the full CSR here) or a square
    float64 array (dense storage).  Products and solves as ``GrmOperator``; the single ones are the k = 1 case of
    the many.  ``csr=(row_ptr, col, val)`` instead of ``grm`` hands a CSR to the library as it is; ``n`` / ``ld``
    override the size and the row stride the library is told (its argument checks are tested this way)."""

    _prefix, _free = "sgx_kmat_", "sgx_kmat_free"

    def __init__(self, grm=None, device: int = 0, csr=None, n: Optional[int] = None, ld: Optional[int] = None):
        L = load()
        h = C.c_void_p()
        if csr is not None:
            rp = np.ascontiguousarray(csr[0], dtype=np.int64)
            col = np.ascontiguousarray(csr[1], dtype=np.int32)
            val = np.ascontiguousarray(csr[2], dtype=np.float64)
            self.n = int(rp.size - 1 if n is None else n)
            self.storage = "csr"
            check(L.sgx_kmat_init_csr(self.n, rp.ctypes.data, col.ctypes.data, val.ctypes.data, int(device), C.byref(h)))
        elif hasattr(grm, "i") and hasattr(grm, "x"):
            self.n = int(grm.n)
            self.storage = "csr"
            rp, col, val = csr_of_upper(self.n, grm.i, grm.j, grm.x)
            check(L.sgx_kmat_init_csr(self.n, rp.ctypes.data, col.ctypes.data, val.ctypes.data, int(device), C.byref(h)))
        else:
            K = np.ascontiguousarray(grm, dtype=np.float64)       # (with ld: [n, ld], the matrix in its first n columns)
            if K.ndim != 2 or (ld is None and K.shape[0] != K.shape[1]):
                raise ValueError("the GRM must be a square matrix")
            self.n = int(K.shape[0] if n is None else n)
            self.storage = "dense"
            check(L.sgx_kmat_init_dense(K.ctypes.data, int(K.shape[1] if ld is None else ld), self.n, int(device),
                                        C.byref(h)))
        self._h = h

    def matvec_ms(self) -> float:
        """Device milliseconds of the kernels of the last product."""
        ms = C.c_double(0)
        check(self._L.sgx_kmat_matvec_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def crossprod(self, b: np.ndarray) -> np.ndarray:
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (self.n,):
            raise ValueError("b must have one entry per sample")
        return self.crossprod_many(b[None, :])[0]

    def pcg_many_dev(self, w_ptr: int, tau, b_ptr: int, ldb: int, k: int, x_ptr: int, maxiter: int = 500,
                     tol: float = 1e-5) -> np.ndarray:
        """Device form of ``pcg_many`` for k <= GRM_MAX_RHS columns: weights at w_ptr, right-hand sides at
        b_ptr + j * ldb doubles, solutions to x_ptr + j * ldb (synchronous) -> iters [k]; bit for bit ``pcg_many``."""
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        iters = np.zeros(max(1, int(k)), dtype=np.int32)
        check(self._L.sgx_kmat_pcg_multi_dev(self._h, w_ptr, tau.ctypes.data, b_ptr, int(ldb), int(k), int(maxiter),
                                             float(tol), x_ptr, iters.ctypes.data))
        return iters[:int(k)]

    def pcg(self, w: np.ndarray, tau, b: np.ndarray, maxiter: int = 500, tol: float = 1e-5):
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (self.n,):
            raise ValueError("b must have one entry per sample")
        X, it = self.pcg_many(w, tau, b[None, :], maxiter, tol)
        return X[0], int(it[0])
