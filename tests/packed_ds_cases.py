"""Packed-real dosage rows for the tests of the stored-rows route -- TEST INFRASTRUCTURE ONLY.

The five classes a dosage node's rows can go to the device in (dPackedReal8U / 8 / 16U / 16, dFloat32), the documented
decoding formula restated in numpy, rows that hold every special case (each class's missing code, an all-missing row,
rows of pure hard calls), and a writer of a SeqArray-style file with such a node.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# class -> (numpy type of the stored value, missing code, scale, offset)
CLASSES = {
    "dPackedReal8U": (np.dtype(np.uint8), 0xFF, 1 / 127, 0.0),
    "dPackedReal8": (np.dtype(np.int8), -128, 1 / 127, 1.0),
    "dPackedReal16U": (np.dtype("<u2"), 0xFFFF, 1e-4, 0.0),
    "dPackedReal16": (np.dtype("<i2"), -32768, 1 / 16384, 1.0),
    "dFloat32": (np.dtype("<f4"), None, 1.0, 0.0),
}

# scales whose stored values decode to dyadic rationals (14 fractional bits at most): the sums of a row are then exact
# in float64 in any order, so AF and mac equal the oracle's sample-by-sample sums bit for bit
DYADIC = {"dPackedReal8U": (1 / 64, 0.0), "dPackedReal8": (1 / 64, 1.0), "dPackedReal16U": (1 / 16384, 0.0),
          "dPackedReal16": (1 / 16384, 1.0), "dFloat32": (1.0, 0.0)}


def decode(raw, cls, scale, offset):
    """The documented formula: dosage = raw * scale + offset, the product rounded and then the sum; the class's
    missing code -> NaN.  float32 rows are widened as they are."""
    dt, miss, _, _ = CLASSES[cls]
    raw = np.asarray(raw, dtype=dt)
    if cls == "dFloat32":
        return raw.astype(np.float64)
    prod = raw.astype(np.float64) * np.float64(scale)
    out = prod + np.float64(offset)
    out[raw == miss] = np.nan
    return out


def encode(x, cls, scale=None, offset=None):
    """Dosages in [0, 2] (NaN = missing) -> the nearest stored value of the class (default: the class's scale / offset
    above; float32 with a scale: on the grid of 2^-14)."""
    dt, miss, s0, o0 = CLASSES[cls]
    if cls == "dFloat32":
        return (x if scale is None else np.rint(x * 16384) / 16384).astype(dt)
    scale, offset = (s0, o0) if scale is None else (scale, offset)
    q = np.rint((np.where(np.isnan(x), 0.0, x) - offset) / scale)
    return np.where(np.isnan(x), miss, q).astype(dt)


def dosages(m, n, seed, codes=None):
    """[m, n] dosages in [0, 2] with 1 % missing: hard calls (``codes``: 0 / 1 / 2 / 3 = missing, else drawn), two rows
    in three blurred; row 1 all missing, rows 0, 3, 6, ... pure hard calls, row 2 without a missing value."""
    rng = np.random.default_rng(seed)
    if codes is None:
        af = 10 ** rng.uniform(-2.0, -0.4, m)
        af[::9] = 1 - af[::9]
        codes = (rng.random((m, n), dtype=np.float32) < af[:, None]).astype(np.uint8)
        codes += (rng.random((m, n), dtype=np.float32) < af[:, None]).astype(np.uint8)
    codes = np.where(rng.random((m, n), dtype=np.float32) < 0.01, 3, codes)
    x = np.where(codes == 3, np.nan, codes.astype(np.float64))
    blur = np.clip(x + rng.normal(0, 0.08, x.shape) * (rng.random(x.shape) < 0.3), 0, 2)
    keep = np.arange(m) % 3 == 0
    x = np.where(keep[:, None], x, blur)
    x[1] = np.nan
    x[2] = np.where(np.isnan(x[2]), 0.0, x[2])
    return x


def stored_rows(cls, x, scale=None, offset=None):
    """``x`` in the class's stored form, every special value present: the missing code (NaN, and for float32 an Inf)."""
    raw = encode(x, cls, scale, offset)
    if cls == "dFloat32":
        raw[0, 0] = np.inf
    return raw


def widen(raw, n_file, seed):
    """The model's samples scattered over a file of ``n_file`` samples: -> (raw_file [m, n_file], sel) with
    raw_file[:, sel] == raw; the other samples hold arbitrary stored values."""
    rng = np.random.default_rng(seed)
    m, n = raw.shape
    sel = rng.permutation(n_file)[:n]
    if raw.dtype.kind == "f":
        wide = rng.random((m, n_file), dtype=np.float32).astype(raw.dtype) * 2
    else:
        info = np.iinfo(raw.dtype)
        wide = rng.integers(info.min, info.max, (m, n_file), dtype=raw.dtype, endpoint=True)
    wide[:, sel] = raw
    return wide, sel


def write_ds_file(path, raw, cls, scale, offset, sample_id, compress="ZIP_RA", ra_block=1 << 16):
    """A SeqArray-style file without a genotype node: sample.id, variant.id, position, chromosome, allele and
    annotation/format/DS (data [variant, sample] of class ``cls``, @data = one value per variant)."""
    from saigegds_amd.gds_write import GdsWriter
    m = raw.shape[0]
    w = GdsWriter(str(path))
    w.put_attr("FileFormat", "SEQ_ARRAY")
    w.add("sample.id", [str(s) for s in sample_id], "none")
    w.add("variant.id", np.arange(1, m + 1), "none")
    w.add("position", np.arange(1, m + 1) * 100, "none")
    w.add("chromosome", ["1"] * m, "none")
    w.add("allele", ["A,C"] * m, "none")
    kw = {} if cls == "dFloat32" else {"scale": scale, "offset": offset}
    w.add("annotation/format/DS/data", np.ascontiguousarray(raw), compress, cls=cls, dims=raw.shape, ra_block=ra_block, **kw)
    w.add("annotation/format/DS/@data", np.ones(m, dtype="<i4").tobytes(), "none", cls="dInt32", dims=(m,))
    w.close()
    return str(path)


def golden_codes(m):
    """Hard calls of the first m variants of grm1k_10k_snp (N = 1000): 0 / 1 / 2, 3 = missing."""
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLDEN, "grm1k_10k_snp.npz"))
    return unpack_dosage_2bit(g["packed"][:m], 1000), [str(s) for s in g["sample_id"]]
