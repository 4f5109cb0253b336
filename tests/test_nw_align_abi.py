"""CPU tests of the alignment-path boundary (da_nw_align_pairs / nw_align / nw_align_strings / clusterconsensus): symbols, the validation
order and texts -- everything is checked before a device is needed, then DA_ERR_NO_DEVICE -- pairs == 0, and the host-only helpers.
No compute calls here."""
import numpy as np
import pytest

import oracle_lib as O

SYMBOLS = ["da_nw_align_pairs", "da_nw_align_workspace_bytes", "da_dev_nw_align_pairs"]
OK, BAD_MATRIX, BAD_RES1, BAD_RES2, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 4, 5, 6, 8, 10, 11


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def raw(lib, x, y, px=None, py=None, pairs=None, matrix=b"BLOSUM62", ld_ops=None, want_ops=True):
    """-> (rc, message, untouched): untouched tells whether every output still holds its fill value"""
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    if pairs is None:
        pairs = len(px) if px is not None else len(x)
    pxa = None if px is None else np.ascontiguousarray(px, np.int32)
    pya = None if py is None else np.ascontiguousarray(py, np.int32)
    if ld_ops is None:
        ld_ops = 254
    ops = np.full((max(pairs, 1), max(ld_ops, 1)), 7, np.uint8)
    ln, mt, sc = (np.full(max(pairs, 1), -7, np.int32) for _ in range(3))
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = lib.da_nw_align_pairs(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), p(pxa), p(pya), pairs,
                               matrix, 10, 4, ops.ctypes.data if want_ops else None, ld_ops, ln.ctypes.data, mt.ctypes.data, sc.ctypes.data)
    untouched = bool((ops == 7).all() and (ln == -7).all() and (mt == -7).all() and (sc == -7).all())
    return rc, (lib.da_last_error().decode("latin-1") if rc else ""), untouched


def test_header_library_and_signatures_agree_on_the_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert lib.da_abi_version() == 2


def test_python_mirror_exports():
    import inspect
    import dynaalign_amd as da
    from dynaalign_amd import device
    sig = inspect.signature(da.nw_align)
    assert list(sig.parameters) == ["x", "y", "matrixName", "gapOpen", "gapExt", "pairs", "ops"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "pairs", "ops")] == ["BLOSUM62", 10, 4, None, True]
    assert sig.parameters["pairs"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ops"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(da.clusterconsensus).parameters)[0] == "df"
    assert callable(da.nw_align_strings) and callable(device.nw_align_pairs)
    assert "center-star" in da.clusterconsensus.__doc__.lower() and "DECIPHER" in da.clusterconsensus.__doc__


def test_workspace_is_whole_wavefronts_of_5_kib_per_pair(lib):
    w = lib.da_nw_align_workspace_bytes
    assert w(0) == 0 and w(1) == w(64) == 64 * 5120 and w(65) == 2 * 64 * 5120 and w(1000) == 16 * 64 * 5120


def test_matrix_name_comes_first(lib):
    # a bad name wins over everything else: bad lists, indices, lengths, residues
    rc, msg, untouched = raw(lib, ["A" * 200, "a"], ["b"], px=[5], py=None, pairs=1, matrix=b"PAM250")
    assert rc == BAD_MATRIX and msg == "Invalid substitution matrix name: PAM250" and untouched


def test_zero_pairs_is_ok_and_writes_nothing(lib):
    rc, msg, untouched = raw(lib, ["a!"], ["?"], px=[], py=[], pairs=0)
    assert rc == OK and untouched
    rc, msg, untouched = raw(lib, [], [], pairs=0)
    assert rc == OK and untouched
    # ... but the matrix name is still looked at
    assert raw(lib, [], [], pairs=0, matrix=b"nope")[0] == BAD_MATRIX


def test_lists_and_indices(lib):
    x, y = ["ACD", "WW"], ["ACD", "KK", "MM"]
    rc, msg, untouched = raw(lib, x, y, px=[0], py=None, pairs=1)
    assert rc == BAD_ARG and "both" in msg and untouched
    rc, msg, untouched = raw(lib, x, y, px=None, py=[0], pairs=1)
    assert rc == BAD_ARG and untouched
    rc, msg, untouched = raw(lib, x, y)                              # the NULL form needs m == n == pairs
    assert rc == BAD_ARG and "m == n == pairs" in msg and untouched
    for px, py in (([0, 2], [0, 0]), ([0, -1], [0, 0]), ([0, 1], [0, 3]), ([0, 1], [-1, 0])):
        rc, msg, untouched = raw(lib, x, y, px=px, py=py)
        assert rc == BAD_ARG and "outside" in msg and untouched, (px, py)
    # an index error wins over a too long sequence, a short ld_ops and a bad residue
    rc, msg, untouched = raw(lib, ["A" * 128, "?"], y, px=[0, 2], py=[0, 0], ld_ops=1)
    assert rc == BAD_ARG and "outside x" in msg and untouched


def test_more_than_127_residues_is_unsupported_and_only_listed_sequences_count(lib):
    x, y = ["A" * 128, "ACD"], ["A" * 127, "C" * 128]
    rc, msg, untouched = raw(lib, x, y, px=[1, 0], py=[0, 0])
    assert rc == UNSUPPORTED and "127" in msg and untouched
    rc, msg, untouched = raw(lib, x, y, px=[1], py=[1])
    assert rc == UNSUPPORTED and "127" in msg and untouched
    # the long ones are not listed: validation passes and only the device is missing; the length wins over ld_ops and residues
    assert raw(lib, x, y, px=[1], py=[0])[0] in (OK, NO_DEVICE)
    rc, msg, _ = raw(lib, ["A" * 128], ["?"], px=[0], py=[0], ld_ops=1)
    assert rc == UNSUPPORTED


def test_ld_ops_must_hold_the_longest_listed_pair(lib):
    x, y = ["ACDEF", "A" * 100], ["ACD", "C" * 100]
    rc, msg, untouched = raw(lib, x, y, px=[0], py=[0], ld_ops=7)
    assert rc == BAD_ARG and "ld_ops = 7" in msg and "8" in msg and untouched
    assert raw(lib, x, y, px=[0], py=[0], ld_ops=8)[0] in (OK, NO_DEVICE)
    assert raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=199)[0] == BAD_ARG
    assert raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=200)[0] in (OK, NO_DEVICE)
    # without ops the leading dimension is not looked at
    assert raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=0, want_ops=False)[0] in (OK, NO_DEVICE)
    # ld_ops wins over a residue error
    assert raw(lib, ["?CD"], ["ACD"], px=[0], py=[0], ld_ops=5)[0] == BAD_ARG


def first_error_by_the_oracle(x, y, px, py):
    """what the reference's lazy fill raises first with the pairs visited p ascending (the oracle runs calc pair by pair)"""
    for i, j in zip(px, py):
        rc, _, _, _, bad = O.nw_pair(x[i], y[j])
        if rc:
            return rc, bad
    return 0, ""


RESIDUE_CASES = [
    (["ACD", "A?D"], ["WW", "K!K"], [0, 1, 1], [0, 0, 1]),      # x[1]'s row 2 error comes before y[1] is ever scanned
    (["ACD", "A?D"], ["WW", "K!K"], [0, 0, 1], [0, 1, 1]),      # pair (0, 1) scans y[1] first
    (["?CD"], ["K!K"], [0], [0]),                                # sequence1[0] before anything of sequence2
    (["A?D"], ["K!K"], [0], [0]),                                # ... but sequence1[1] after all of sequence2
    (["", "ACD"], ["K!K", "WW"], [0, 1], [0, 1]),                # an empty sequence1 checks nothing; y[0] is never scanned again
    (["A?D"], [""], [0], [0]),                                   # an empty sequence2 still has sequence1 checked
    (["ACD", "b"], ["WW", "z"], [0], [0]),                       # sequences that are not listed are not checked
    (["AC!"], ["WW"], [0, 0], [0, 0]),
]


@pytest.mark.parametrize("x,y,px,py", RESIDUE_CASES)
def test_residue_errors_are_the_lazy_fills_first(lib, x, y, px, py):
    want_rc, bad = first_error_by_the_oracle(x, y, px, py)
    rc, msg, untouched = raw(lib, x, y, px=px, py=py)
    if want_rc == 0:
        assert rc in (OK, NO_DEVICE)
        return
    assert want_rc in (O.ERR_BAD_RES1, O.ERR_BAD_RES2)
    assert rc == want_rc and untouched
    assert msg == "Invalid amino acid in sequence%d: %s" % (1 if rc == BAD_RES1 else 2, bad)


def test_the_residue_cases_cover_both_errors_and_none():
    got = {first_error_by_the_oracle(*c)[0] for c in RESIDUE_CASES}
    assert got == {0, O.ERR_BAD_RES1, O.ERR_BAD_RES2}


def test_null_form_checks_pair_p_with_p(lib):
    rc, msg, _ = raw(lib, ["ACD", "WW"], ["KK", "M?"])
    assert rc == BAD_RES2 and msg.endswith("sequence2: ?")


def test_valid_input_fails_loudly_without_a_device(lib):
    x, y, px, py = ["ACD", ""], ["", "WW"], [0, 1, 1], [1, 0, 1]
    if lib.da_device_count() > 0:
        rc, msg, untouched = raw(lib, x, y, px=px, py=py)
        assert rc == OK and not untouched
        return
    rc, msg, untouched = raw(lib, x, y, px=px, py=py)
    assert rc == NO_DEVICE and untouched and "no CPU fallback" in msg
    assert raw(lib, x, y, px=px, py=py, want_ops=False)[0] == NO_DEVICE
    assert raw(lib, ["ACD", "W"], ["", "WW"])[0] == NO_DEVICE


def test_nw_align_requires_equal_lengths_without_pairs():
    import dynaalign_amd as da
    with pytest.raises(ValueError, match="same length"):
        da.nw_align(["ACD", "WW"], ["ACD"])
    with pytest.raises(ValueError, match="same length"):
        da.nw_align(["ACD"], ["ACD"], pairs=([0, 0], [0]))


def test_nw_align_raises_the_librarys_errors(built):
    import dynaalign_amd as da
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align(["ACD"], ["ACD"], "PAM250")
    assert e.value.code == BAD_MATRIX and str(e.value) == "Invalid substitution matrix name: PAM250"
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align(["A" * 128], ["ACD"])
    assert e.value.code == UNSUPPORTED
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align(["ACD"], ["ACD"], pairs=([1], [0]))
    assert e.value.code == BAD_ARG
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align(["ACD"], ["AzD"])
    assert e.value.code == BAD_RES2 and str(e.value) == "Invalid amino acid in sequence2: z"
    r = da.nw_align([], [])                                           # nothing listed: empty results, no device needed
    assert r.ops == [] and r.length.shape == (0,) and r.matches.shape == (0,) and r.score.shape == (0,)
    assert da.nw_align(["ACD"], ["ACD"], pairs=([], []), ops=False).ops is None


def test_clusterconsensus_of_single_member_clusters_needs_no_device(built):
    import dynaalign_amd as da
    assert da.clusterconsensus([("ACD", "2.1"), ("WWW", "1.1")]) == [("2.1", "ACD"), ("1.1", "WWW")]
    assert da.clusterconsensus(np.array([["ACD", "2.1"]], dtype=object)) == [("2.1", "ACD")]
    assert da.clusterconsensus([]) == []
    with pytest.raises(da.DynaAlignError) as e:                       # two members: the library's length limit speaks first
        da.clusterconsensus([("A" * 128, 1), ("ACD", 1)])
    assert e.value.code == UNSUPPORTED


def test_clusterconsensus_host_logic_equals_the_model_when_the_alignments_are_the_models(monkeypatch):
    """the tallying, the centre choice and the tie rules of the package's clusterconsensus, with nw_align answered by the model"""
    import dynaalign_amd as da
    import nw_align_model as model
    from dynaalign_amd import similarity

    def fake(x, y, matrixName="BLOSUM62", gapOpen=10, gapExt=4, *, pairs=None, ops=True):
        r = [model.align(x[i], y[j], matrixName, gapOpen, gapExt) for i, j in zip(*pairs)]
        return similarity.NWAlignment([t[0] for t in r] if ops else None, np.array([t[1] for t in r], np.int32),
                                      np.array([t[2] for t in r], np.int32), np.array([t[3] for t in r], np.int32))

    monkeypatch.setattr(similarity, "nw_align", fake)
    core = "MKTAYIAKQRQISFVK"
    rows = [("KKKKCKKK", "t"), ("W" + core, "g"), ("RKKKAKKK", "t"), ("ACDE", 1), (core[:3] + "W" + core[4:], "g"), ("KRKKAKKK", "t"),
            ("ACDF", 1), ("KKRKSKKK", "t"), (core[:9] + "W" + core[10:], "g"), ("KKKRSKKK", "t"), ("WWWW", "single"), ("", "e"), ("", "e")]
    want = [("t", "KKKKAKKK"), ("g", core), (1, "ACDE"), ("single", "WWWW"), ("e", "")]
    assert model.consensus(rows) == want
    assert da.clusterconsensus(rows) == want
    rng = np.random.default_rng(3)
    rows = []
    for c in range(8):
        root = model.random_seq(rng, 12)
        rows += [(model.mutate(rng, root, rate=0.3), c) for _ in range(1 + c)]
    assert da.clusterconsensus(rows) == model.consensus(rows)


def test_nw_align_strings():
    import dynaalign_amd as da
    assert da.nw_align_strings("PPPSYETVMAAA", "TPPPSYETVMAA", "LDDDDDDDDDUDD") == ("-PPPSYETVMAAA", "TPPPSYETVM-AA")
    ga, gb = da.nw_align_strings("ACACCA", "CAACAC", "UDLDDLDU")
    assert len(ga) == len(gb) == 8 and ga.replace("-", "") == "ACACCA" and gb.replace("-", "") == "CAACAC"
    assert [i for i, ch in enumerate(gb) if ch == "-"] == [0, 7] and [i for i, ch in enumerate(ga) if ch == "-"] == [2, 5]
    assert da.nw_align_strings("", "", "") == ("", "")
    assert da.nw_align_strings("", "AC", "LL") == ("--", "AC") and da.nw_align_strings("AC", "", "UU") == ("AC", "--")
    with pytest.raises(ValueError):
        da.nw_align_strings("AC", "AC", "D")                          # the path does not reach the ends
    with pytest.raises(ValueError):
        da.nw_align_strings("AC", "AC", "DX")
