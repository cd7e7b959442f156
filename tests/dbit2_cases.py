"""Shared by tests/test_dbit2_raw.py and tests/test_gpu_dbit2.py: allele indices with every kind of row the dBit2 decoder
has to get right, files written from them, and a numpy decoder of the stored bytes written from the rule alone."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ALL_MISSING, MONOMORPHIC, ALT_MAJOR, TWO_ROWS, THREE_ROWS = 1, 2, 3, 10, 20


def alleles(m, n, seed):
    """Allele indices [m, n, 2] (0 = reference, -1 = missing): sites of one row with allele codes 0 / 1 / 2 at minor
    allele frequencies from 1 % to 50 %, about 1 % of the samples with one or both alleles missing; row 1 all missing,
    row 2 monomorphic, row 3 with alt as the major allele; row 10 a site of two stored rows (indices up to 14) and row 20
    one of three (up to 62), both with samples that are missing (all digits 3) and samples whose index has a digit 3 in
    one row only (3, 7, 12, 48: not missing)."""
    rng = np.random.default_rng(seed)
    af = 10 ** rng.uniform(-2.0, -0.3, m)
    af[ALT_MAJOR] = 0.9
    al = (rng.random((m, n, 2)) < af[:, None, None]).astype(np.int64)
    al[(al == 1) & (rng.random((m, n, 2)) < 0.2)] = 2                    # allele code 2 counts as non-reference
    one = rng.random((m, n)) < 0.007
    al[one, rng.integers(0, 2, int(one.sum()))] = -1                     # one allele missing
    al[rng.random((m, n)) < 0.004] = -1                                  # both
    al[ALL_MISSING] = -1
    al[MONOMORPHIC] = 0
    for v, top, odd in ((TWO_ROWS, 14, (3, 7, 12, 13)), (THREE_ROWS, 62, (3, 12, 48, 15, 51, 60))):
        if v >= m:
            continue
        x = np.where(rng.random((n, 2)) < 0.3, rng.integers(1, top + 1, (n, 2)), 0)
        x[rng.random((n, 2)) < 0.1] = rng.choice(odd, 1)[0]
        x[rng.random(n) < 0.02] = -1
        x[3], x[4] = (-1, 1), (-1, -1)
        for k, o in enumerate(odd):                                      # each of them in one allele of a sample, with a plain partner
            x[5 + 2 * k] = (o, k % 3)
        x[0], x[-1] = (top, 0), (0, top)                                 # (the site keeps its number of rows)
        al[v] = x
    return al


def codes_of(al):
    """$dosage_alt of allele indices: 3 if an allele is missing, else the number of non-reference alleles."""
    c = (al > 0).sum(axis=-1).astype(np.uint8)
    c[(al < 0).any(axis=-1)] = 3
    return c


def nibbles(data, bit0, count):
    """`count` nibbles of the bytes `data` from bit `bit0` on, low nibble of a byte first."""
    d = np.asarray(data, dtype=np.uint8)
    nb = np.empty(2 * d.size, dtype=np.uint8)
    nb[0::2], nb[1::2] = d & 15, d >> 4
    return nb[bit0 // 4:bit0 // 4 + count]


def to_bytes(nb, bit0=0):
    """The inverse: nibbles -> bytes, the first one at bit `bit0` of the first byte."""
    nb = np.concatenate([np.zeros(bit0 // 4, np.uint8), np.asarray(nb, dtype=np.uint8)])
    if nb.size % 2:
        nb = np.concatenate([nb, np.zeros(1, np.uint8)])
    return (nb[0::2] | (nb[1::2] << 4)).astype(np.uint8)


def decode(data, bit0, n_file, n_rows, m, sel=None):
    """The rule of the issue, in numpy: per sample a nibble, a0 in bits 0-1 and a1 in bits 2-3; over a variant's rows an
    allele is missing when every digit is 3 and non-reference when a digit is non-zero and it is not missing; code 3 if
    an allele is missing, else the number of non-reference alleles; LSB first, four samples a byte."""
    reps = np.ones(m, dtype=np.int64) if n_rows is None else np.asarray(n_rows, dtype=np.int64)
    nb = nibbles(data, bit0, int(reps.sum()) * n_file).reshape(-1, n_file)
    row0 = np.concatenate([[0], np.cumsum(reps)])
    n_out = n_file if sel is None else len(sel)
    out = np.zeros((m, (n_out + 3) // 4), dtype=np.uint8)
    for j in range(m):
        rows = nb[row0[j]:row0[j + 1]]
        code = np.zeros(n_file, dtype=np.uint8)
        miss = np.zeros(n_file, dtype=bool)
        for shift in (0, 2):
            dig = (rows >> shift) & 3
            m_a = (dig == 3).all(axis=0)
            code += ((dig != 0).any(axis=0) & ~m_a).astype(np.uint8)
            miss |= m_a
        code[miss] = 3
        if sel is not None:
            code = code[np.asarray(sel)]
        code = np.concatenate([code, np.zeros((-n_out) % 4, np.uint8)]).reshape(-1, 4)
        out[j] = code[:, 0] | (code[:, 1] << 2) | (code[:, 2] << 4) | (code[:, 3] << 6)
    return out


def write_file(path, al, sample_id=None, compress="none", ra_block=4096):
    from saigegds_amd.gds_write import write_seqarray_alleles
    write_seqarray_alleles(str(path), al, sample_id=sample_id, compress=compress, ra_block=ra_block)
    return str(path)


def tile(data, bit0, n_file, n_rows, m, times):
    """The same variants `times` times over -> (bytes from bit 0, n_rows or None, variants)"""
    reps = np.ones(m, dtype=np.int64) if n_rows is None else np.asarray(n_rows, dtype=np.int64)
    nb = nibbles(data, bit0, int(reps.sum()) * n_file)
    return to_bytes(np.tile(nb, times)), None if n_rows is None else np.tile(reps, times).astype(np.int32), m * times
