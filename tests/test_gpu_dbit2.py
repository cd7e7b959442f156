"""genotype/data rows through the C ABI as the file stores them (sgx_scan_dbit2, sgx_block_load_dbit2): decoded and
sample-selected on the device.  The reference is always sgx_scan_2bit / sgx_block_load on the host decoder's rows of the
same bytes (GdsFile.dosage_alt_packed_range: sgx_decode_dbit2, _dosage_alt_multirow for sites of several rows), compared
with np.array_equal on the bits of out8 and on valid."""
import os

import numpy as np
import pytest

import dbit2_cases as D
from conftest import GOLDEN, assert_table_close, load_null_model, scan_model

pytestmark = pytest.mark.gpu

M = 300
MODELS = ["saige_model.npz", "saige_model_quant.npz"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    yield


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(o, v, ro, rv):
    return np.array_equal(v, rv) and np.array_equal(_bits(o), _bits(ro))


def _selections(n_file, n=1000):
    rng = np.random.default_rng(n_file)
    if n_file == n:
        return None
    if n_file == 1037:                                     # shuffled, non-monotone
        return rng.permutation(n_file)[:n]
    return np.delete(np.arange(n_file), 500)[:n]           # 1000 of 1001, in the file's order


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """n_file -> (GdsFile, allele indices): M + 1 variants, so that [1, M + 1) of an odd n_file starts on a half byte"""
    from saigegds_amd.gds import GdsFile
    d = tmp_path_factory.mktemp("dbit2")
    out = {}
    for n_file in (1000, 1037, 1001):
        al = D.alleles(M + 1, n_file, n_file)
        g = GdsFile(D.write_file(d / f"a{n_file}.gds", al))
        g.genotype_dims()
        out[n_file] = (g, al)
    return out


def _case(files, n_file, v0=0, sel="default"):
    """(raw, bit0, n_rows, sel, host-decoded rows) of variants [v0, v0 + M)"""
    g, _ = files[n_file]
    if isinstance(sel, str):
        sel = _selections(n_file)
    raw, bit0, n_rows = g.genotype_raw_range(v0, v0 + M)
    ref_rows = g.dosage_alt_packed_range(v0, v0 + M, sel)
    assert n_rows is not None and sorted(set(n_rows.tolist())) == [1, 2, 3]
    return raw, bit0, n_rows, sel, ref_rows


def _check(sc, raw, bit0, n_file, n_rows, sel, ref_rows, what, m=M):
    ro, rv = sc.scan_2bit(ref_rows)
    o, v = sc.scan_dbit2(raw, bit0, n_file, n_rows, sel, m)
    bad = np.flatnonzero((_bits(o) != _bits(ro)).any(axis=1) | (v != rv))
    print(what, "variants", m, "valid", int(rv.sum()), "rows that differ", bad[:10].tolist())
    assert _same(o, v, ro, rv), what
    return o, v


@pytest.mark.parametrize("model", MODELS)
def test_d1_scan_dbit2_equals_scan_2bit(files, model):
    """All 1000 of 1000 (no selection); 1000 of 1037 shuffled (rows start off every alignment and on half bytes); 1000 of
    1001 with bit0 = 4; a selection with the file's first and last sample.  The rows hold codes 0 / 1 / 2, missing
    alleles, an all-missing, a monomorphic and an alt-major row, a 2-row and a 3-row site."""
    from saigegds_amd._lib import Scanner
    sm = scan_model(model)
    with Scanner(sm, device=0) as sc:
        for n_file, v0 in ((1000, 0), (1037, 0), (1037, 1), (1001, 1)):
            raw, bit0, n_rows, sel, ref_rows = _case(files, n_file, v0)
            assert bit0 == (4 if v0 and n_file % 2 else 0)
            assert np.array_equal(D.decode(raw, bit0, n_file, n_rows, M, sel), ref_rows)      # the rule, the host decoder
            o, v = _check(sc, raw, bit0, n_file, n_rows, sel, ref_rows, f"{model} {n_file} from {v0}")
            assert 100 < v.sum() < M and not v[D.ALL_MISSING - v0] and not v[D.MONOMORPHIC - v0]
            assert v[D.ALT_MAJOR - v0] and o[D.ALT_MAJOR - v0, 0] > 0.8
            if n_file == 1000:
                assert v[D.TWO_ROWS] and v[D.THREE_ROWS]
        # the file's first and last sample among the selected, no index twice
        rng = np.random.default_rng(4)
        sel = np.concatenate([[1036, 0], rng.permutation(np.arange(1, 1036))[:998]])
        assert np.unique(sel).size == 1000
        raw, bit0, n_rows, sel, ref_rows = _case(files, 1037, 1, sel)
        _check(sc, raw, bit0, 1037, n_rows, sel, ref_rows, f"{model} first and last sample")
        # variants of one row each (n_rows = NULL)
        g = files[1037][0]
        raw, bit0, n_rows = g.genotype_raw_range(D.THREE_ROWS + 1, M + 1)
        assert n_rows is None
        sel = _selections(1037)
        _check(sc, raw, bit0, 1037, None, sel, g.dosage_alt_packed_range(D.THREE_ROWS + 1, M + 1, sel), f"{model} one row each", M - D.THREE_ROWS)


def test_d2_multirow_sites_against_the_allele_indices(files):
    """The rows the reference decodes from the 2-row and 3-row site are the codes of the allele indices they were written
    from: all digits 3 is missing, a digit 3 in one row only is not."""
    from saigegds_amd.gds import pack_dosage_2bit, unpack_dosage_2bit
    g, al = files[1037]
    for v in (D.TWO_ROWS, D.THREE_ROWS):
        codes = D.codes_of(al[v])
        assert (codes == 3).sum() > 5 and ((al[v] == 3).any(axis=1) & (codes != 3)).sum() >= 1
        assert np.array_equal(unpack_dosage_2bit(g._dosage_alt_multirow(v, v + 1, None, None, 1 << 20), 1037)[0], codes)
        raw, bit0, n_rows = g.genotype_raw_range(v, v + 1)
        assert n_rows.tolist() == [2 if v == D.TWO_ROWS else 3]
        assert np.array_equal(D.decode(raw, bit0, 1037, n_rows, 1), pack_dosage_2bit(codes[None, :]))


@pytest.mark.parametrize("n", [13, 997])
def test_d3_small_models(files, tmp_path, n):
    """n_samp = 13 (below one output dword) and 997 (the tail dword partly filled) out of the 1037-sample file: the
    padding of the decoded rows does not disturb the table."""
    from saigegds_amd._lib import Scanner
    ids = load_null_model("saige_model.npz").sample_id
    rng = np.random.default_rng(n)
    sm = scan_model("saige_model.npz", mac=1.0 if n == 13 else 4.0, sample_ids=[ids[i] for i in np.sort(rng.permutation(1000)[:n])])
    assert sm.n == n
    sel = rng.permutation(1037)[:n]
    with Scanner(sm, device=0) as sc:
        for v0 in (0, 1):
            raw, bit0, n_rows, sel, ref_rows = _case(files, 1037, v0, sel)
            o, v = _check(sc, raw, bit0, 1037, n_rows, sel, ref_rows, f"n_samp {n} from {v0}")
            assert v.sum() > 10
    if n == 997:                                            # ... and without a selection, rows of 997 samples
        from saigegds_amd.gds import GdsFile
        g, al = files[1037]
        sub = GdsFile(D.write_file(tmp_path / "a997.gds", al[:, 40:, :]))
        sub.genotype_dims()
        raw, bit0, n_rows = sub.genotype_raw_range(1, M + 1)
        with Scanner(sm, device=0) as sc:
            _check(sc, raw, bit0, 997, n_rows, None, sub.dosage_alt_packed_range(1, M + 1), "n_samp 997, no selection")


def test_d4_chunks(files):
    """pipe_mb = 1 is 4096 rows of the 256-byte stride: 28 x 300 variants are two whole chunks and a tail, cut where
    sgx_scan_2bit cuts the decoded rows, and give the bits of the one-chunk call."""
    from saigegds_amd._lib import Scanner
    sm = scan_model("saige_model.npz")
    with Scanner(sm, device=0) as sc:
        for n_file in (1000, 1037):
            raw, bit0, n_rows, sel, ref_rows = _case(files, n_file, 1)
            big, reps, m = D.tile(raw, bit0, n_file, n_rows, M, 28)
            ref_big = np.ascontiguousarray(np.tile(ref_rows, (28, 1)))
            assert m == 8400 > 2 * ((1 << 20) // sc.row_stride())
            sc.set_option("pipe_mb", 0)
            one, one_valid = sc.scan_dbit2(big, 0, n_file, reps, sel, m)
            sc.set_option("pipe_mb", 1)
            o, v = _check(sc, big, 0, n_file, reps, sel, ref_big, f"chunks, {n_file}", m)
            assert _same(o, v, one, one_valid)
            assert _same(o[:M], v[:M], o[-M:], v[-M:])
            sc.set_option("pipe_mb", 0)


def _dev_out(m):
    import torch
    return (torch.full((m, 8), -1.0, dtype=torch.float64, device="cuda:0"), torch.zeros(m, dtype=torch.uint8, device="cuda:0"))


def test_d5_block(files):
    """load_dbit2 then scan_block equals load_block of the host-decoded rows then scan_block, with two models."""
    from saigegds_amd._lib import Block, Scanner
    tabs = {}
    with Block(1000, M) as ref_blk, Block(1000, M) as blk:
        for n_file, v0 in ((1000, 0), (1037, 1)):
            raw, bit0, n_rows, sel, ref_rows = _case(files, n_file, v0)
            for model in MODELS:
                with Scanner(scan_model(model), device=0) as sc:
                    if model == MODELS[0]:                  # loaded with the first model's handle, scanned with both
                        sc.load_block(ref_blk, ref_rows)
                        blk.load_dbit2(sc, raw, bit0, n_file, n_rows, sel, M)
                        assert blk.n_variants == ref_blk.n_variants == M
                    for b, key in ((ref_blk, "ref"), (blk, "dev")):
                        o, v = _dev_out(M)
                        sc.scan_block(b, o.data_ptr(), v.data_ptr())
                        sc.sync()
                        tabs[key] = (o.cpu().numpy(), v.cpu().numpy())
                    assert _same(*tabs["dev"], *tabs["ref"]), (n_file, model)
                    assert tabs["ref"][1].sum() > 100
                    rm, rm_valid = sc.scan_2bit(ref_rows)
                    assert np.array_equal(rm_valid, tabs["dev"][1])


def test_d5_block_loads_in_three_chunks(files):
    """pipe_mb = 1 is 4096 rows of the block's 256-byte stride: the 8400 variants of test_d4_chunks are loaded in three
    chunks, the third into the pipeline buffer of the first.  load_block of the host-decoded rows and load_dbit2 of the
    stored bytes then give, through scan_block, the table of the one-chunk load_block; each load is made twice in a row,
    so that a call finds both buffers used by the one before."""
    from saigegds_amd._lib import Block, Scanner
    sm = scan_model("saige_model.npz")
    with Scanner(sm, device=0) as sc:
        try:
            for n_file in (1000, 1037):
                raw, bit0, n_rows, sel, ref_rows = _case(files, n_file, 1)
                big, reps, m = D.tile(raw, bit0, n_file, n_rows, M, 28)
                ref_big = np.ascontiguousarray(np.tile(ref_rows, (28, 1)))
                assert m == 8400 > 2 * ((1 << 20) // sc.row_stride())
                tabs = {}
                for key, pipe_mb in (("host rows, one chunk", 0), ("host rows", 1), ("stored bytes", 1)):
                    sc.set_option("pipe_mb", pipe_mb)
                    with Block(1000, m) as blk:
                        for _ in range(2):
                            if key == "stored bytes":
                                blk.load_dbit2(sc, big, 0, n_file, reps, sel, m)
                            else:
                                sc.load_block(blk, ref_big)
                        assert blk.n_variants == 8400
                        o, v = _dev_out(m)
                        sc.scan_block(blk, o.data_ptr(), v.data_ptr())
                        sc.sync()
                    tabs[key] = (o.cpu().numpy(), v.cpu().numpy())
                    print(n_file, key, "valid", int(tabs[key][1].sum()))
                one = tabs["host rows, one chunk"]
                assert one[1].sum() > 100
                assert _same(*tabs["host rows"], *one), n_file
                assert _same(*tabs["stored bytes"], *one), n_file
        finally:
            sc.set_option("pipe_mb", 0)


def test_d6_golden_file_through_the_driver(golden_bin, monkeypatch):
    """seqAssocGLMM_SPA on grm1k_10k_snp.gds with GENOTYPE_DECODE = "device": the first 2 000 variants reproduce
    saige_pval.npz, and the table equals the "host" run bit for bit."""
    from saigegds_amd import assoc
    mod = load_null_model("saige_model.npz")
    path = os.path.join(GOLDEN, "grm1k_10k_snp.gds")
    ans = {}
    for mode in ("device", "host"):
        monkeypatch.setattr(assoc, "GENOTYPE_DECODE", mode)
        monkeypatch.setattr(assoc, "BLOCK_SIZE", 3000)      # four blocks, the reader one ahead of the scan
        tm = {}
        ans[mode] = assoc.seqAssocGLMM_SPA(path, mod, mac=4, verbose=False, timing=tm)
        assert tm["decoded_bytes"] == 10000 * (500 if mode == "device" else 250)
    dev = ans["device"]
    assert len(dev["id"]) == 10000
    k = 2000
    cols = ("AF.alt", "mac", "num", "beta", "SE", "pval", "p.norm", "converged")
    out = np.stack([np.asarray(dev[c], dtype=np.float64)[:k] for c in cols], axis=1)
    ref = np.stack([np.asarray(golden_bin[c], dtype=np.float64)[:k] for c in ("AF_alt", "mac", "num", "beta", "SE", "pval", "p_norm", "converged")], axis=1)
    assert_table_close(out, np.ones(k, np.uint8), ref, np.ones(k, np.uint8), what="golden, decoded on the device")
    for c in cols:
        assert np.array_equal(_bits(dev[c]), _bits(ans["host"][c])), c


def test_d7_bad_arguments_leave_the_handle_usable(files):
    from saigegds_amd import _lib
    from saigegds_amd._lib import Block, Scanner, SgxError
    L = _lib.load()
    sm = scan_model("saige_model.npz")
    raw0, bit00, n_rows0, _, ref0 = _case(files, 1000, 0)
    raw, bit0, n_rows, sel, ref_rows = _case(files, 1037, 1)
    bad_hi, bad_lo = sel.copy(), sel.copy()
    bad_hi[17], bad_lo[999] = 1037, -1
    rows_0, rows_17 = n_rows.copy(), n_rows.copy()
    rows_0[5], rows_17[7] = 0, 17
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    s32, r32 = i32(sel), i32(n_rows)
    with Scanner(sm, device=0) as sc, Block(1000, M) as blk:
        ref, ref_valid = sc.scan_2bit(ref_rows)
        out, valid = np.empty((M, 8)), np.zeros(M, dtype=np.uint8)
        raw_scan = lambda a, b0, nfs, nr, s: _lib.check(L.sgx_scan_dbit2(  # noqa: E731
            sc._h, a, b0, nfs, nr, s, M, out.ctypes.data, valid.ctypes.data))
        cases = [
            ("NULL buffer", lambda: raw_scan(None, 4, 1037, r32.ctypes.data, s32.ctypes.data)),
            ("NULL buffer", lambda: _lib.check(L.sgx_scan_dbit2(sc._h, raw.ctypes.data, 4, 1037, r32.ctypes.data, s32.ctypes.data, M,
                                                                None, valid.ctypes.data))),
            ("bit0", lambda: raw_scan(raw.ctypes.data, 2, 1037, r32.ctypes.data, s32.ctypes.data)),
            ("bit0", lambda: raw_scan(raw.ctypes.data, 8, 1037, r32.ctypes.data, s32.ctypes.data)),
            ("n_file_samp", lambda: raw_scan(raw.ctypes.data, 4, 999, r32.ctypes.data, s32.ctypes.data)),
            ("no selection", lambda: sc.scan_dbit2(raw, bit0, 1037, n_rows, None, M)),
            ("outside the file", lambda: sc.scan_dbit2(raw, bit0, 1037, n_rows, bad_hi, M)),
            ("outside the file", lambda: sc.scan_dbit2(raw, bit0, 1037, n_rows, bad_lo, M)),
            ("1 to 16 rows", lambda: raw_scan(raw.ctypes.data, 4, 1037, i32(rows_0).ctypes.data, s32.ctypes.data)),
            ("1 to 16 rows", lambda: raw_scan(raw.ctypes.data, 4, 1037, i32(rows_17).ctypes.data, s32.ctypes.data)),
            ("NULL buffer", lambda: _lib.check(L.sgx_block_load_dbit2(sc._h, blk._b, None, 4, 1037, r32.ctypes.data, s32.ctypes.data, M))),
            ("bit0", lambda: _lib.check(L.sgx_block_load_dbit2(sc._h, blk._b, raw.ctypes.data, 1, 1037, r32.ctypes.data, s32.ctypes.data, M))),
            ("no selection", lambda: blk.load_dbit2(sc, raw, bit0, 1037, n_rows, None, M)),
            ("outside the file", lambda: blk.load_dbit2(sc, raw, bit0, 1037, n_rows, bad_hi, M)),
            ("1 to 16 rows", lambda: _lib.check(L.sgx_block_load_dbit2(sc._h, blk._b, raw.ctypes.data, 4, 1037, i32(rows_17).ctypes.data,
                                                                       s32.ctypes.data, M))),
            ("holds up to", lambda: blk.load_dbit2(sc, *D.tile(raw, bit0, 1037, n_rows, M, 2)[:1], 0, 1037,
                                                   np.tile(n_rows, 2), sel, 2 * M)),
        ]
        for msg, call in cases:
            with pytest.raises(SgxError, match=msg) as ei:
                call()
            assert ei.value.code == -1, msg                 # SGX_EINVAL
        with pytest.raises(ValueError, match="too short"):
            sc.scan_dbit2(raw[:-1], bit0, 1037, n_rows, sel, M)
        o1, v1 = sc.scan_dbit2(raw, bit0, 1037, n_rows, sel, M)           # the handle still scans, and correctly
        blk.load_dbit2(sc, raw, bit0, 1037, n_rows, sel, M)
        o, v = _dev_out(M)
        sc.scan_block(blk, o.data_ptr(), v.data_ptr())
        sc.sync()
        with Block(1000, M) as ref_blk:
            sc.load_block(ref_blk, ref_rows)
            o3, v3 = _dev_out(M)
            sc.scan_block(ref_blk, o3.data_ptr(), v3.data_ptr())
            sc.sync()
        assert _same(o.cpu().numpy(), v.cpu().numpy(), o3.cpu().numpy(), v3.cpu().numpy())
    assert _same(o1, v1, ref, ref_valid) and ref_valid.sum() > 100
