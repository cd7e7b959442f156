"""The pseudo-variant of a group of 2-bit rows in numpy, and the constructed ultra-rare rows of the
driver tests.  Nothing here works on packed words: the rows are unpacked to one code a sample, the group's
minor-allele dosages are stacked, the per-sample ``max`` is taken and the result is packed again."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def minor_dosage(codes, flip):
    """[m, n] codes 0..3 -> the minor-allele dosage: the code, 2 - code where the row is flipped, 0 where missing."""
    codes = np.asarray(codes, dtype=np.int64)
    d = np.where(np.asarray(flip, dtype=bool)[:, None], 2 - codes, codes)
    return np.where(codes == 3, 0, d)


def collapse_ref(packed, n_samp, grp_ptr, var_idx, flip):
    """-> (rows [n_groups, bpv] uint8: codes 0, 1, 2, zeros beyond sample n_samp - 1; counts [n_groups, 2] int32)."""
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    packed = np.asarray(packed, dtype=np.uint8)
    var_idx, flip = np.asarray(var_idx, dtype=np.int64), np.asarray(flip)
    ng = len(grp_ptr) - 1
    rows, counts = np.zeros((ng, packed.shape[1]), dtype=np.uint8), np.zeros((ng, 2), dtype=np.int32)
    for g in range(ng):
        a, b = int(grp_ptr[g]), int(grp_ptr[g + 1])
        if a == b:
            continue
        top = minor_dosage(unpack_dosage_2bit(packed[var_idx[a:b]], n_samp), flip[a:b]).max(axis=0)
        rows[g, :(n_samp + 3) // 4] = pack_dosage_2bit(top[None, :].astype(np.uint8))[0]
        counts[g] = (top == 1).sum(), (top == 2).sum()
    return rows, counts


def counts_of(codes):
    """[m, n] codes -> (n non-missing, s their sum, mac, flip = s > n: the scan's)."""
    ok = codes != 3
    n, s = ok.sum(axis=1), np.where(ok, codes, 0).sum(axis=1)
    return n, s, np.minimum(s, 2 * n - s), s > n


# ---- the driver tests' data -----------------------------------------------------------------------------------------

N_GOLD, N_RARE = 120, 36


def rare_rows(n_samp=1000, seed=11):
    """N_RARE constructed rows with 1 .. 10 minor alleles (row k: 1 + k % 10), every third alt-major (the carriers hold
    codes 1 / 0 in a row of 2s), every fourth with 1 .. 3 % missing codes, hets and homs mixed."""
    rng = np.random.default_rng(seed)
    codes = np.zeros((N_RARE, n_samp), dtype=np.uint8)
    for k in range(N_RARE):
        mac = 1 + k % 10
        n_hom = int(rng.integers(0, mac // 2 + 1)) if k % 2 else 0
        who = rng.choice(n_samp, mac - n_hom, replace=False)      # n_hom homs and mac - 2 n_hom hets: mac minor alleles
        codes[k, who[:n_hom]] = 2
        codes[k, who[n_hom:]] = 1
        if k % 3 == 2:
            codes[k] = 2 - codes[k]
        if k % 4 == 3:
            free = np.setdiff1d(np.arange(n_samp), who)
            codes[k, rng.choice(free, int(rng.integers(10, 31)), replace=False)] = 3
    return codes


def driver_case(trait):
    """The first N_GOLD golden variants (N = 1000) followed by ``rare_rows``; 1-based units of every shape: without an
    ultra-rare member, with one, with many, of ultra-rare members only (one and many), empty, and two units sharing
    rare rows -> (codes [m, 1000], the null model, units, sample ids)."""
    from conftest import load_null_model
    from saigegds_amd.gds import unpack_dosage_2bit
    g = np.load(os.path.join(GOLD, "grm1k_10k_snp.npz"))
    codes = np.concatenate([unpack_dosage_2bit(g["packed"][:N_GOLD], 1000), rare_rows()])
    mod = load_null_model("saige_model.npz" if trait == "binary" else "saige_model_quant.npz")
    r0 = N_GOLD + 1                                             # 1-based index of the first constructed row
    units = [np.arange(1, 31),                                  # golden rows only (some of them may be rare themselves)
             np.concatenate([np.arange(31, 51), [r0]]),         # one ultra-rare member
             np.concatenate([[r0 + 1, r0 + 2], np.arange(51, 71), np.arange(r0 + 3, r0 + 12)]),   # many, not at the end
             np.arange(r0 + 12, r0 + 30),                       # only ultra-rare members
             np.array([r0 + 30]),                               # a single one
             np.zeros(0, dtype=np.int64),
             np.concatenate([np.arange(71, 121), np.arange(r0 + 8, r0 + 36)])]   # shares rare rows with units 2 and 3
    return codes, mod, units, [str(s) for s in g["sample_id"]]


def stored_case(codes, units, collapse_mac):
    """The source the driver's result with ``collapse_mac`` is compared with: the reference's pseudo-rows stored as real
    variants after all original rows, the units naming their common variants and then their pseudo-row -> (codes, units,
    n.collapsed, the pseudo-rows' codes per unit or None)."""
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    n, s, mac, flip = counts_of(codes)
    # a variant in the test: mac > 0 (with thresholds 0 / 0 / 1 the scan keeps such a row unless every genotype is missing)
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
        row, _ = collapse_ref(pack_dosage_2bit(codes), codes.shape[1], [0, u.size], u, flip[u])
        pseudo.append(unpack_dosage_2bit(row, codes.shape[1])[0])
        new_units.append(np.concatenate([r[~rare] + 1, [codes.shape[0] + sum(p is not None for p in pseudo)]]))
    extra = [p for p in pseudo if p is not None]
    return (np.concatenate([codes, np.array(extra, dtype=np.uint8)]) if extra else codes), new_units, np.array(n_coll), pseudo
