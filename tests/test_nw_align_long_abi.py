"""CPU tests of the long alignment-path boundary (da_nw_align_long_pairs / da_dev_nw_align_long_pairs / nw_align_long / the align_fn hook of
clusterconsensus): the mirror of tests/test_nw_align_abi.py -- the same validation order, codes and texts, everything checked before a
device is needed, then DA_ERR_NO_DEVICE -- with the length limit at 1024 residues, plus the workspace size and the device-pointer call's
argument checks.  No compute calls here."""
import numpy as np
import pytest

import oracle_lib as O
from test_nw_align_abi import RESIDUE_CASES, first_error_by_the_oracle

SYMBOLS = ["da_nw_align_long_pairs", "da_nw_align_long_workspace_bytes", "da_dev_nw_align_long_pairs"]
OK, BAD_MATRIX, BAD_RES1, BAD_RES2, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 4, 5, 6, 8, 10, 11


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def raw(lib, x, y, px=None, py=None, pairs=None, matrix=b"BLOSUM62", ld_ops=None, want_ops=True, entry="da_nw_align_long_pairs"):
    """-> (rc, message, untouched): untouched tells whether every output still holds its fill value"""
    xr, xo = O.pack(x)
    yr, yo = O.pack(y)
    if pairs is None:
        pairs = len(px) if px is not None else len(x)
    pxa = None if px is None else np.ascontiguousarray(px, np.int32)
    pya = None if py is None else np.ascontiguousarray(py, np.int32)
    if ld_ops is None:
        ld_ops = 2048
    ops = np.full((max(pairs, 1), max(ld_ops, 1)), 7, np.uint8)
    ln, mt, sc = (np.full(max(pairs, 1), -7, np.int32) for _ in range(3))
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    rc = getattr(lib, entry)(xr.ctypes.data, xo.ctypes.data, len(x), yr.ctypes.data, yo.ctypes.data, len(y), p(pxa), p(pya), pairs,
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
    assert "nw_align_long" in da.__all__
    sig = inspect.signature(da.nw_align_long)
    assert sig == inspect.signature(da.nw_align)
    assert list(sig.parameters) == ["x", "y", "matrixName", "gapOpen", "gapExt", "pairs", "ops"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "pairs", "ops")] == ["BLOSUM62", 10, 4, None, True]
    assert sig.parameters["pairs"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ops"].kind is inspect.Parameter.KEYWORD_ONLY
    cc = inspect.signature(da.clusterconsensus).parameters
    assert list(cc) == ["df", "matrixName", "gapOpen", "gapExt", "align_fn"]
    assert cc["align_fn"].default is None and cc["align_fn"].kind is inspect.Parameter.KEYWORD_ONLY
    dev = inspect.signature(device.nw_align_long_pairs).parameters
    assert list(dev)[:2] == ["dx", "dy"] and list(dev)[-6:] == ["pair_x", "pair_y", "ops", "ld_ops", "max_len", "work"]
    assert dev["max_len"].default is None and dev["work"].default is None
    assert callable(device.nw_align_long_workspace_bytes)


def test_workspace_is_capped_slots_of_max_len_plus_63_steps(lib):
    w = lib.da_nw_align_long_workspace_bytes
    assert w(0, 500) == 0 and w(-1, 500) == 0 and w(5, -1) == 0
    assert w(1, 0) == 63 * 256 and w(1, 566) == (566 + 63) * 256 and w(1, 1024) == (1024 + 63) * 256
    assert w(7, 300) == 7 * (300 + 63) * 256
    # non-decreasing in both arguments ...
    grid_p = [1, 2, 63, 64, 65, 1000, 3071, 3072, 3073, 10 ** 4, 10 ** 6, 10 ** 9]
    grid_l = [0, 1, 127, 128, 566, 1023, 1024, 1025, 5000]
    for l in grid_l:
        vals = [w(p, l) for p in grid_p]
        assert vals == sorted(vals) and vals[0] > 0, l
    for p in grid_p:
        vals = [w(p, l) for l in grid_l]
        assert vals == sorted(vals), p
    # ... and no growth with the pairs beyond the cap on resident wavefronts
    cap = w(10 ** 9, 566) // w(1, 566)
    assert 256 <= cap <= 8192 and w(cap, 566) == w(cap + 1, 566) == w(10 ** 12, 566) == cap * w(1, 566)
    assert w(cap - 1, 566) < w(cap, 566)


def test_matrix_name_comes_first(lib):
    # a bad name wins over everything else: bad lists, indices, lengths, residues
    rc, msg, untouched = raw(lib, ["A" * 2000, "a"], ["b"], px=[5], py=None, pairs=1, matrix=b"PAM250")
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
    rc, msg, untouched = raw(lib, ["A" * 1025, "?"], y, px=[0, 2], py=[0, 0], ld_ops=1)
    assert rc == BAD_ARG and "outside x" in msg and untouched


@pytest.mark.parametrize("x,y,px,py,ld", [
    (["ACD", "WW"], ["ACD", "KK", "MM"], [0], None, None), (["ACD", "WW"], ["ACD", "KK", "MM"], None, None, None),
    (["ACD", "WW"], ["ACD", "KK", "MM"], [0, 2], [0, 0], None), (["ACD", "WW"], ["ACD", "KK", "MM"], [0, 1], [-1, 0], None),
    (["ACDEF", "A" * 100], ["ACD", "C" * 100], [0], [0], 7), (["?CD"], ["K!K"], [0], [0], None), (["A?D"], ["K!K"], [0], [0], None),
    (["ACD"], ["ACD"], [0], [0], None),
])
def test_codes_and_texts_are_those_of_da_nw_align_pairs(lib, x, y, px, py, ld):
    """below the short call's own limit the two calls refuse the same input with the same code and the same words"""
    pairs = 1 if px is not None and py is None else None
    a = raw(lib, x, y, px=px, py=py, pairs=pairs, ld_ops=ld if ld is not None else 254)
    b = raw(lib, x, y, px=px, py=py, pairs=pairs, ld_ops=ld if ld is not None else 254, entry="da_nw_align_pairs")
    assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2] or a[0] == OK)
    # ... and at the length check they differ in the number alone
    a = raw(lib, ["A" * 1025], ["ACD"], px=[0], py=[0])
    b = raw(lib, ["A" * 1025], ["ACD"], px=[0], py=[0], entry="da_nw_align_pairs")
    assert a[0] == b[0] == UNSUPPORTED and a[1] == b[1].replace("127", "1024")


def test_1024_residues_pass_1025_are_unsupported_and_only_listed_sequences_count(lib):
    x, y = ["A" * 1025, "ACD", "C" * 1024], ["A" * 1024, "C" * 1025]
    rc, msg, untouched = raw(lib, x, y, px=[1, 0], py=[0, 0])
    assert rc == UNSUPPORTED and "1024" in msg and "127" not in msg and untouched
    rc, msg, untouched = raw(lib, x, y, px=[1], py=[1])
    assert rc == UNSUPPORTED and "1024" in msg and untouched
    # 1024 residues on either side and on both pass the length check: only the device is missing
    for px, py in (([1], [0]), ([2], [0]), ([2, 1], [0, 0])):
        assert raw(lib, x, y, px=px, py=py)[0] in (OK, NO_DEVICE), (px, py)
    # 128 residues, which da_nw_align_pairs refuses, pass
    assert raw(lib, ["A" * 128], ["C" * 128], px=[0], py=[0])[0] in (OK, NO_DEVICE)
    # the length wins over ld_ops and residues
    rc, msg, _ = raw(lib, ["A" * 1025], ["?"], px=[0], py=[0], ld_ops=1)
    assert rc == UNSUPPORTED


def test_ld_ops_must_hold_the_longest_listed_pair(lib):
    x, y = ["ACDEF", "A" * 700], ["ACD", "C" * 600]
    rc, msg, untouched = raw(lib, x, y, px=[0], py=[0], ld_ops=7)
    assert rc == BAD_ARG and "ld_ops = 7" in msg and "8" in msg and untouched
    assert raw(lib, x, y, px=[0], py=[0], ld_ops=8)[0] in (OK, NO_DEVICE)
    rc, msg, untouched = raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=1299)
    assert rc == BAD_ARG and "1300" in msg and untouched
    assert raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=1300)[0] in (OK, NO_DEVICE)
    # without ops the leading dimension is not looked at
    assert raw(lib, x, y, px=[0, 1], py=[0, 1], ld_ops=0, want_ops=False)[0] in (OK, NO_DEVICE)
    # ld_ops wins over a residue error
    assert raw(lib, ["?CD"], ["ACD"], px=[0], py=[0], ld_ops=5)[0] == BAD_ARG


LONG_RESIDUE_CASES = [
    (["A" * 300 + "?" + "C" * 200], ["K" * 500 + "!"], [0], [0]),    # sequence1[300] comes after all of sequence2
    (["?" + "A" * 600], ["K" * 500 + "!"], [0], [0]),                # sequence1[0] before anything of sequence2
    (["A" * 1024, "AC?"], ["W" * 1024, "K" * 200 + "z"], [0, 1, 1], [0, 0, 1]),
    (["A" * 200], ["W" * 1000, "z" * 1024], [0], [0]),               # sequences that are not listed are not checked
]


@pytest.mark.parametrize("x,y,px,py", RESIDUE_CASES + LONG_RESIDUE_CASES)
def test_residue_errors_are_the_lazy_fills_first(lib, x, y, px, py):
    want_rc, bad = first_error_by_the_oracle(x, y, px, py)
    rc, msg, untouched = raw(lib, x, y, px=px, py=py)
    if want_rc == 0:
        assert rc in (OK, NO_DEVICE)
        return
    assert want_rc in (O.ERR_BAD_RES1, O.ERR_BAD_RES2)
    assert rc == want_rc and untouched
    assert msg == "Invalid amino acid in sequence%d: %s" % (1 if rc == BAD_RES1 else 2, bad)


def test_the_long_residue_cases_cover_both_errors_and_none():
    got = {first_error_by_the_oracle(*c)[0] for c in LONG_RESIDUE_CASES}
    assert got == {0, O.ERR_BAD_RES1, O.ERR_BAD_RES2}


def test_null_form_checks_pair_p_with_p(lib):
    rc, msg, _ = raw(lib, ["ACD", "W" * 300], ["KK", "M" * 400 + "?"])
    assert rc == BAD_RES2 and msg.endswith("sequence2: ?")


def test_valid_input_fails_loudly_without_a_device(lib):
    x, y, px, py = ["ACD", "", "A" * 200], ["", "WW", "C" * 1024], [0, 1, 1, 2, 0], [1, 0, 1, 2, 2]
    if lib.da_device_count() > 0:
        rc, msg, untouched = raw(lib, x, y, px=px, py=py)
        assert rc == OK and not untouched
        return
    rc, msg, untouched = raw(lib, x, y, px=px, py=py)
    assert rc == NO_DEVICE and untouched and "no CPU fallback" in msg
    assert raw(lib, x, y, px=px, py=py, want_ops=False)[0] == NO_DEVICE
    assert raw(lib, ["ACD", "W", "K" * 128], ["", "WW", "C"])[0] == NO_DEVICE


def dev_raw(lib, m=2, n=2, px=1, py=1, pairs=2, matrix_id=0, ops=1, ld_ops=600, max_len=300, work=1, work_bytes=None, codes=1):
    """da_dev_nw_align_long_pairs on made-up addresses (nothing is dereferenced before a device is required) -> (rc, message)"""
    fake = 1 << 20
    if work_bytes is None:
        work_bytes = lib.da_nw_align_long_workspace_bytes(1, max_len) if max_len >= 0 else 0
    rc = lib.da_dev_nw_align_long_pairs(fake * codes or None, fake * codes or None, m, fake, fake, n, fake * px or None, fake * py or None, pairs,
                                        matrix_id, 10, 4, fake * ops or None, ld_ops, fake, fake, fake, max_len, fake * work or None, work_bytes,
                                        None)
    return rc, (lib.da_last_error().decode("latin-1") if rc else "")


def test_device_pointer_call_checks_its_arguments_without_a_device(lib):
    assert dev_raw(lib, pairs=-1)[0] == BAD_ARG and dev_raw(lib, m=-1)[0] == BAD_ARG
    assert dev_raw(lib, pairs=0, codes=0)[0] == OK                           # nothing listed
    rc, msg = dev_raw(lib, px=1, py=0)
    assert rc == BAD_ARG and "both" in msg
    rc, msg = dev_raw(lib, px=0, py=0, m=2, n=3)
    assert rc == BAD_ARG and "m == n == pairs" in msg
    assert dev_raw(lib, codes=0)[0] == BAD_ARG
    assert dev_raw(lib, ld_ops=-1)[0] == BAD_ARG
    rc, msg = dev_raw(lib, max_len=-1)
    assert rc == BAD_ARG and "max_len" in msg
    # the workspace must hold one slot of (max_len + 63) * 256 bytes when ops are wanted ...
    one = lib.da_nw_align_long_workspace_bytes(1, 300)
    rc, msg = dev_raw(lib, work_bytes=one - 1)
    assert rc == BAD_ARG and "slot" in msg and "da_nw_align_long_workspace_bytes" in msg
    assert dev_raw(lib, work=0)[0] == BAD_ARG
    # ... and every check has passed with exactly one slot, or with no workspace when no ops are wanted
    if lib.da_device_count() == 0:
        assert dev_raw(lib, work_bytes=one)[0] == NO_DEVICE
        assert dev_raw(lib, ops=0, work=0, work_bytes=0)[0] == NO_DEVICE


def test_nw_align_long_raises_the_value_errors_of_nw_align():
    import dynaalign_amd as da
    with pytest.raises(ValueError, match="same length"):
        da.nw_align_long(["ACD", "WW"], ["ACD"])
    with pytest.raises(ValueError, match="same length"):
        da.nw_align_long(["ACD"], ["ACD"], pairs=([0, 0], [0]))
    for args, kw in (((["ACD", "WW"], ["ACD"]), {}), ((["ACD"], ["ACD"]), {"pairs": ([0, 0], [0])})):
        with pytest.raises(ValueError) as a:
            da.nw_align(*args, **kw)
        with pytest.raises(ValueError) as b:
            da.nw_align_long(*args, **kw)
        assert str(a.value) == str(b.value)


def test_nw_align_long_raises_the_librarys_errors(built):
    import dynaalign_amd as da
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align_long(["ACD"], ["ACD"], "PAM250")
    assert e.value.code == BAD_MATRIX and str(e.value) == "Invalid substitution matrix name: PAM250"
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align_long(["A" * 1025], ["ACD"])
    assert e.value.code == UNSUPPORTED and "1024" in str(e.value)
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align_long(["ACD"], ["ACD"], pairs=([1], [0]))
    assert e.value.code == BAD_ARG
    with pytest.raises(da.DynaAlignError) as e:
        da.nw_align_long(["A" * 500], ["A" * 300 + "z"])
    assert e.value.code == BAD_RES2 and str(e.value) == "Invalid amino acid in sequence2: z"
    r = da.nw_align_long([], [])                                      # nothing listed: empty results, no device needed
    assert r.ops == [] and r.length.shape == (0,) and r.matches.shape == (0,) and r.score.shape == (0,)
    assert da.nw_align_long(["ACD"], ["ACD"], pairs=([], []), ops=False).ops is None


def test_clusterconsensus_calls_align_fn_with_the_documented_arguments(built):
    """a recording stub that answers with the model: two calls over one pool, pairs as index lists, ops False then True"""
    import dynaalign_amd as da
    import nw_align_model as model
    from dynaalign_amd import similarity
    calls = []

    def stub(*args, **kw):
        calls.append((args, kw))
        x, y, matrix, go, ge = args
        r = [model.align(x[i], y[j], matrix, go, ge) for i, j in zip(*kw["pairs"])]
        return similarity.NWAlignment([t[0] for t in r] if kw["ops"] else None, np.array([t[1] for t in r], np.int32),
                                      np.array([t[2] for t in r], np.int32), np.array([t[3] for t in r], np.int32))

    rng = np.random.default_rng(11)
    root = model.random_seq(rng, 140)
    rows = [(model.mutate(rng, root, max_len=2000), "long"), ("ACDEFGHIK", "short"), (model.mutate(rng, root, max_len=2000), "long"), ("WWWW", "one"),
            ("ACDEFGHIR", "short"), (model.mutate(rng, root, max_len=2000), "long"), ("ACDFGHIK", "short")]
    assert max(len(r[0]) for r in rows) > 127
    got = da.clusterconsensus(rows, matrixName="BLOSUM80", gapOpen=7, gapExt=2, align_fn=stub)
    assert got == model.consensus(rows, aligner=lambda a, b: model.align(a, b, "BLOSUM80", 7, 2))
    assert len(calls) == 2
    pool = [rows[0][0], rows[2][0], rows[5][0], rows[1][0], rows[4][0], rows[6][0]]          # clusters of two or more, first-appearance order
    for (args, kw), want_ops in zip(calls, (False, True)):
        assert len(args) == 5 and args[0] == pool and args[1] is args[0] and args[2:] == ("BLOSUM80", 7, 2)
        assert sorted(kw) == ["ops", "pairs"] and kw["ops"] is want_ops
        pi, pj = kw["pairs"]
        assert len(pi) == len(pj) and all((i < 3) == (j < 3) and i != j for i, j in zip(pi, pj))
    assert len(calls[0][1]["pairs"][0]) == 12 and len(calls[1][1]["pairs"][0]) == 4
    # defaults reach the hook too
    calls.clear()
    da.clusterconsensus(rows, align_fn=stub)
    assert [c[0][2:] for c in calls] == [("BLOSUM62", 10, 4)] * 2
    # a call without clusters of two or more never aligns
    calls.clear()
    assert da.clusterconsensus([("A" * 500, 1), ("C" * 300, 2)], align_fn=stub) == [(1, "A" * 500), (2, "C" * 300)] and not calls


def test_without_align_fn_clusterconsensus_still_refuses_128_residues(built):
    import dynaalign_amd as da
    with pytest.raises(da.DynaAlignError) as e:
        da.clusterconsensus([("A" * 128, 1), ("ACD", 1)])
    assert e.value.code == UNSUPPORTED and "127" in str(e.value)
    with pytest.raises(da.DynaAlignError) as e:
        da.clusterconsensus([("A" * 128, 1), ("ACD", 1)], align_fn=None)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(da.DynaAlignError) as e:                          # the long call has its own limit
        da.clusterconsensus([("A" * 1025, 1), ("ACD", 1)], align_fn=da.nw_align_long)
    assert e.value.code == UNSUPPORTED and "1024" in str(e.value)
