"""Cases of the dosage -> hard-call quantiser (sgx_quantize_packed, the fit on a dosage-only file) -- TEST INFRASTRUCTURE ONLY.

Its own numpy statement of the rule (the GPU tests compare against this one, not against the package's
``gds.quantize_dosage_2bit``), the edge rows -- every rounding boundary a class can represent, at known positions --
and the rows of the parity tests.  Built on ``packed_ds_cases``.
"""
import math

import numpy as np

import packed_ds_cases as P

# decoded value -> expected code, the boundaries of C's round (halves away from zero) and of the range 0 .. 2
EDGE_VALUES = [(-0.5, 3), (-0.484375, 0), (0.0, 0), (0.484375, 0), (0.5, 1), (1.484375, 1), (1.5, 2), (2.484375, 2),
               (2.5, 3), (3.96875, 3)]
_F = np.float32
# float32 only: the non-finite values, values far outside an int, a denormal, the float32 just below each half
EDGE_VALUES_F32 = [(_F(-0.0), 0), (_F(np.nan), 3), (_F(np.inf), 3), (_F(-np.inf), 3), (_F(1e30), 3), (_F(-1e30), 3),
                   (_F(1e-45), 0), (np.nextafter(_F(0.5), _F(0)), 0), (np.nextafter(_F(1.5), _F(0)), 1),
                   (np.nextafter(_F(2.5), _F(0)), 2)]


def ref_codes(v):
    """3 where v is not finite, else r = C's round(v) -- the truncation, moved one away from zero where the (exact)
    remainder is at least a half -- if r is 0, 1 or 2, else 3."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    x = np.where(fin, v, 0.0)
    t = np.trunc(x)
    r = t + np.sign(x) * (np.abs(x - t) >= 0.5)
    code = np.full(v.shape, 3, dtype=np.uint8)
    for k in (0, 1, 2):
        code[fin & (r == k)] = k
    return code


def ref_pack(codes):
    """Four samples a byte, sample 4 b + k in bits 2 k .. 2 k + 1, the last byte's missing samples as 0."""
    m, n = codes.shape
    out = np.zeros((m, (n + 3) // 4), dtype=np.uint8)
    for i in range(n):
        out[:, i // 4] |= (codes[:, i].astype(np.uint8) & 3) << (2 * (i % 4))
    return out


def ref_quantize(raw, cls, scale, offset, sel=None):
    """-> (packed, n_valid, allele_sum, ds_valid, ds_sum, sum_abs): the expected outputs of the quantiser on stored
    rows; ds_sum of an integer class from the exact integer sum, of float32 the correctly rounded sum (math.fsum);
    sum_abs = the sum of |v| over the finite dosages (the scale of float32's bound)."""
    dt, miss, _, _ = P.CLASSES[cls]
    raw = np.asarray(raw, dtype=dt)
    x = raw if sel is None else raw[:, np.asarray(sel)]
    v = P.decode(x, cls, scale, offset)
    fin = np.isfinite(v)
    codes = ref_codes(v)
    ok = codes != 3
    nv = ok.sum(axis=1).astype(np.int32)
    sm = np.where(ok, codes, 0).sum(axis=1).astype(np.int32)
    dv = fin.sum(axis=1).astype(np.int32)
    ds = np.zeros(x.shape[0])
    sa = np.zeros(x.shape[0])
    for j in range(x.shape[0]):
        if cls == "dFloat32":
            ds[j] = math.fsum(v[j][fin[j]].tolist())
        else:
            tot = int(x[j][fin[j]].astype(np.int64).sum())
            ds[j] = np.float64(float(tot)) * np.float64(scale) + np.float64(float(dv[j])) * np.float64(offset)
        sa[j] = math.fsum(np.abs(v[j][fin[j]]).tolist())
    return ref_pack(codes), nv, sm, dv, ds, sa


def edge_list(cls):
    """[(stored value, expected code)] of the class with its DYADIC scale: the boundaries it can represent, then its
    missing code (float32: NaN is among its extras)."""
    dt, miss, _, _ = P.CLASSES[cls]
    scale, offset = P.DYADIC[cls]
    out = []
    for v, code in EDGE_VALUES:
        if cls == "dFloat32":
            out.append((_F(v), code))
            continue
        q = (v - offset) / scale
        info = np.iinfo(dt)
        if q == int(q) and info.min <= q <= info.max and int(q) != miss:
            out.append((dt.type(int(q)), code))
    if cls == "dFloat32":
        out += EDGE_VALUES_F32
    else:
        out.append((dt.type(miss), 3))
    return out


def edge_rows(cls, n):
    """-> (raw [k, n], where): the edge values of the class, spread over one row (n at least their number: a stride
    apart, so they fall into different bytes and dwords, the last of them on the row's last sample) or laid row after
    row over as many rows as they need; the other samples hold a stored 0.  where: [(row, column, expected code)]."""
    dt = P.CLASSES[cls][0]
    e = edge_list(cls)
    k = (len(e) + n - 1) // n
    raw = P.encode(np.zeros((k, n)), cls, *P.DYADIC[cls])
    where = []
    for i, (val, code) in enumerate(e):
        if k == 1:
            r, c = 0, (n - 1 if i == len(e) - 1 else i * (n // len(e)))
        else:
            r, c = divmod(i, n)
        raw[r, c] = val
        where.append((r, c, code))
    return raw.astype(dt), where


def parity_rows(cls, n, seed):
    """The rows of a parity case at n samples: 7 rows of ``dosages()``, the edge row(s), an all-missing row and a row
    of pure hard calls, in the class's stored form with its DYADIC scale.
    -> (raw, scale, offset, where), where = the edge values' (row, column, expected code)."""
    scale, offset = P.DYADIC[cls]
    rng = np.random.default_rng(seed + 1)
    body = P.stored_rows(cls, P.dosages(7, n, seed), scale, offset)
    edge, where = edge_rows(cls, n)
    extra = np.vstack([np.full((1, n), np.nan), rng.integers(0, 3, (1, n)).astype(np.float64)])
    raw = np.vstack([body, edge, P.encode(extra, cls, scale, offset)])
    return np.ascontiguousarray(raw), scale, offset, [(7 + r, c, code) for r, c, code in where]
