"""The pseudo-variant of a group of dosage rows in numpy, written from the definition, and the driver
tests' data: the rows of ``collapse_ref.driver_case`` turned into real dosages.  Nothing here is shared with the kernel.

Per sample i of group U:   top_i = +0.0;  for e in U:  x = row_e[i];  v = missing(x) ? 0 : (flip_e ? 2 - x : x);
                           if v > top_i: top_i = v
uint8 rows: 0xFF is missing and 2 - x is integer arithmetic; rows held as doubles (float64 and int32 input): non-finite
is missing and 2 - x one rounded subtraction.  The strict comparison keeps negative values, -0.0 and NaN out."""
import numpy as np

import collapse_ref as CR

NA_INT = np.iinfo(np.int32).min


def resident(rows):
    """Rows as a dosage block holds them: uint8 as they are, int32 as doubles (NA_INTEGER -> NaN), float64 as they are."""
    rows = np.asarray(rows)
    if rows.dtype == np.int32:
        return np.where(rows == NA_INT, np.nan, rows.astype(np.float64))
    assert rows.dtype in (np.uint8, np.float64)
    return rows


def minor_dosage(row, flip):
    """One resident row -> v per sample (int64 for uint8 rows, float64 else)."""
    if row.dtype == np.uint8:
        x = row.astype(np.int64)
        return np.where(row == 0xFF, 0, 2 - x if flip else x)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(row), np.float64(2.0) - row if flip else row, 0.0)


def collapse_ds_ref(rows, grp_ptr, var_idx, flip):
    """rows [m, n] in resident form -> the pseudo-rows [n_groups, n] in the same form."""
    rows = resident(rows)
    u8 = rows.dtype == np.uint8
    out = np.zeros((len(grp_ptr) - 1, rows.shape[1]), dtype=rows.dtype)
    for g in range(len(grp_ptr) - 1):
        top = np.zeros(rows.shape[1], dtype=np.int64 if u8 else np.float64)
        for e in range(int(grp_ptr[g]), int(grp_ptr[g + 1])):
            v = minor_dosage(rows[var_idx[e]], bool(flip[e]))
            top = np.where(v > top, v, top)
        out[g] = top
    return out


def counts_of(rows):
    """Resident rows -> (n non-missing, s their sum, mac = min(s, 2n - s), flip = s > n: the scan's)."""
    rows = resident(rows)
    ok = rows != 0xFF if rows.dtype == np.uint8 else np.isfinite(rows)
    n = ok.sum(axis=1)
    s = np.where(ok, rows, 0).astype(np.float64).sum(axis=1)
    return n, s, np.minimum(s, 2 * n - s), s > n


# ---- the driver tests' data -----------------------------------------------------------------------------------------

def driver_case(trait, kind, seed=5):
    """``collapse_ref.driver_case`` as dosages -> (rows [m, 1000], the null model, units, sample ids).
    kind "f64": the golden rows become imputed-like values in [0, 2] (a third of the genotypes moved off their hard call,
    two decimals), the constructed rare rows keep exact zeros for non-carriers and get carriers at fractional dosages
    (0.6, 0.9 or 1.2 times the hard call by row, jittered by a tenth and capped at 2, so that the real mac of the rows built
    with 9 and 10 minor alleles falls on both sides of 10); alt-major rows stay alt-major (2 - x) and missing codes
    become NaN.
    kind "u8": the hard calls as bytes (0xFF missing) with a few values of 3, which keep the matrix a dosage input: in
    two common golden rows and at one carrier of two constructed rows (one of them alt-major, where 2 - 3 never enters)."""
    codes, mod, units, ids = CR.driver_case(trait)
    miss = codes == 3
    if kind == "u8":
        rows = np.where(miss, 0xFF, codes).astype(np.uint8)
        for r in (3, 40):
            rows[r, np.flatnonzero(rows[r] == 1)[:2]] = 3
        for r in (CR.N_GOLD + 4, CR.N_GOLD + 5):                 # (row N_GOLD + 5 is alt-major: k % 3 == 2)
            carrier = np.flatnonzero((codes[r] != 3) & (codes[r] != (2 if (r - CR.N_GOLD) % 3 == 2 else 0)))
            rows[r, carrier[0]] = 3
        return rows, mod, units, ids
    assert kind == "f64"
    rng = np.random.default_rng(seed)
    x = np.where(miss, 0, codes).astype(np.float64)
    alt = CR.counts_of(codes)[3]
    minor = np.where(alt[:, None], 2 - x, x)                     # dosage of the minor allele
    g = slice(0, CR.N_GOLD)
    moved = rng.random(minor[g].shape) < 1 / 3
    minor[g] = np.clip(minor[g] + moved * rng.normal(0, 0.15, minor[g].shape), 0, 2)
    r = slice(CR.N_GOLD, None)
    scale = np.array([0.6, 0.9, 1.2])[(np.arange(CR.N_RARE) // 10) % 3]                  # rows 20 .. 29: mac up to 12
    minor[r] = minor[r] * scale[:, None] * rng.uniform(0.9, 1.1, minor[r].shape)
    minor = np.minimum(np.rint(minor * 100) / 100, 2.0)
    rows = np.where(alt[:, None], 2 - minor, minor)
    rows[miss] = np.nan
    return rows, mod, units, ids


def stored_case(rows, units, collapse_mac):
    """The source the driver's result with ``collapse_mac`` is compared with (``collapse_ref.stored_case`` for dosages):
    the reference's pseudo-rows stored as real variants after all original rows, the units naming their common variants
    and then their pseudo-row -> (rows, units, n.collapsed, the pseudo-row per unit or None)."""
    n, s, mac, flip = counts_of(rows)
    assert not (np.abs(mac - collapse_mac) < 1e-6).any() or rows.dtype == np.uint8   # no real mac on the cut-off itself
    new_units, pseudo, n_coll = [], [], []
    for ix in units:
        r = np.asarray(ix, dtype=np.int64) - 1
        rare = (mac[r] > 0) & (mac[r] <= collapse_mac)
        n_coll.append(int(rare.sum()))
        if not rare.any():
            new_units.append(np.asarray(ix, dtype=np.int64))
            pseudo.append(None)
            continue
        u = r[rare]
        pseudo.append(collapse_ds_ref(rows, [0, u.size], u, flip[u])[0])
        new_units.append(np.concatenate([r[~rare] + 1, [rows.shape[0] + sum(p is not None for p in pseudo)]]))
    extra = [p for p in pseudo if p is not None]
    return (np.concatenate([rows, np.array(extra, dtype=rows.dtype)]) if extra else rows), new_units, np.array(n_coll), pseudo
