"""CPU tests of the device consensus boundary (da_cluster_consensus / clusterconsensus_device): symbols, clusters of one, and the
validation order and texts -- everything is checked before a device is needed, and every error is the one
``clusterconsensus(rows, align_fn=nw_align_long)`` raises on the same rows.  No compute calls here."""
import inspect

import numpy as np
import pytest

SYMBOLS = ["da_cluster_consensus", "da_dev_cluster_consensus", "da_dev_cluster_consensus_workspace_bytes", "da_dev_consensus_center_sums",
           "da_dev_consensus_pick", "da_dev_consensus_vote"]
OK, BAD_MATRIX, BAD_RES1, BAD_RES2, NO_DEVICE, UNSUPPORTED, BAD_ARG = 0, 4, 5, 6, 8, 10, 11


@pytest.fixture(scope="module")
def lib(built):
    from dynaalign_amd import _capi
    return _capi.load()


def test_header_library_and_signatures_agree_on_the_symbols(lib):
    from dynaalign_amd import _capi
    declared = _capi.header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(_capi.SIGNATURES) == declared
    assert "(the cluster-consensus entry points -- da_cluster_consensus," in open(_capi.HEADER_PATH).read()      # the preamble's "likewise" line


def test_python_mirror_exports():
    import dynaalign_amd as da
    from dynaalign_amd import device
    sig = inspect.signature(da.clusterconsensus_device)
    assert list(sig.parameters) == ["df", "matrixName", "gapOpen", "gapExt", "return_centers"]
    assert [sig.parameters[p].default for p in ("matrixName", "gapOpen", "gapExt", "return_centers")] == ["BLOSUM62", 10, 4, False]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("matrixName", "gapOpen", "gapExt", "return_centers"))
    doc = da.clusterconsensus_device.__doc__
    assert "center-star" in doc.lower() and "``clusterconsensus``" in doc and "nw_align_long" in doc
    assert "clusterconsensus_device" in da.__all__
    for name in ("cluster_consensus", "consensus_center_sums", "consensus_pick", "consensus_vote", "cluster_consensus_workspace_bytes"):
        assert callable(getattr(device, name)), name


def test_clusters_of_one_need_no_device(built):
    import dynaalign_amd as da
    for rows in ([("ACD", "2.1"), ("WWW", "1.1")], [], [("A?D", 7)], [("", "e")], [("A" * 1025, 1), ("ACD", 2)]):
        assert da.clusterconsensus_device(rows) == da.clusterconsensus(rows), rows
    assert da.clusterconsensus_device(np.array([["ACD", "2.1"]], dtype=object)) == [("2.1", "ACD")]
    assert da.clusterconsensus_device({"clustered_seq": np.array([["ACD", "2.1"], ["WW", "x"]], dtype=object)}) == [("2.1", "ACD"), ("x", "WW")]
    # ... where the matrix name is never looked at either, as in clusterconsensus
    assert da.clusterconsensus_device([("ACD", 1)], matrixName="PAM250") == da.clusterconsensus([("ACD", 1)], matrixName="PAM250")
    got, centers = da.clusterconsensus_device([("ACD", "b"), ("W?", "a"), ("KK", "c")], return_centers=True)
    assert got == [("b", "ACD"), ("a", "W?"), ("c", "KK")] and centers == [0, 1, 2]


VALIDATION_CASES = {
    "a bad residue at position 0 of member 0": [("?CD", 1), ("ACD", 1), ("AC!", 1)],
    "position 1 of member 0, member 1 bad too: member 1's seq2 error": [("A?D", 1), ("K!K", 1), ("ACD", 1)],
    "an empty member 0 and a bad member 1": [("", 1), ("AC!", 1), ("ACD", 1)],
    "an empty member 0 and a member 1 bad at 0": [("", 1), ("!CD", 1), ("z", 1)],
    "a clean member 0 meets the first bad member": [("ACD", 1), ("WW", 1), ("Kb", 1), ("K!", 1)],
    "a bad residue only in the second cluster": [("ACD", 1), ("ACE", 1), ("WW", 2), ("W?W", 2)],
    "a bad residue in both clusters: the first cluster's": [("ACD", 1), ("ACx", 1), ("WW", 2), ("W?W", 2)],
    "clusters interleaved: first appearance decides": [("W?W", "b"), ("ACx", "a"), ("WW", "b"), ("ACD", "a")],
    "1025 residues in a cluster of two": [("ACD", 1), ("ACE", 1), ("WW", 2), ("K", 2), ("A" * 1025, 2)],
    "1025 residues as member 0": [("A" * 1025, 2), ("WW", 2), ("K", 2)],
    "1025 residues win over a bad residue": [("?", 1), ("A" * 1025, 1)],
    "an unknown matrix name": [("ACD", 1), ("ACE", 1)],
    "an unknown matrix name wins over everything": [("?" * 1025, 1), ("ACE", 1)],
}


@pytest.mark.parametrize("what", sorted(VALIDATION_CASES))
def test_errors_are_those_of_clusterconsensus_with_nw_align_long(built, what):
    import dynaalign_amd as da
    rows = VALIDATION_CASES[what]
    matrix = "PAM250" if "matrix" in what else "BLOSUM62"
    with pytest.raises(da.DynaAlignError) as want:
        da.clusterconsensus(rows, matrixName=matrix, align_fn=da.nw_align_long)
    with pytest.raises(da.DynaAlignError) as got:
        da.clusterconsensus_device(rows, matrixName=matrix)
    assert want.value.code in (BAD_MATRIX, BAD_RES1, BAD_RES2, UNSUPPORTED)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), what


def test_the_validation_cases_cover_every_error():
    import dynaalign_amd as da
    codes = set()
    for what, rows in VALIDATION_CASES.items():
        with pytest.raises(da.DynaAlignError) as e:
            da.clusterconsensus(rows, matrixName="PAM250" if "matrix" in what else "BLOSUM62", align_fn=da.nw_align_long)
        codes.add(e.value.code)
    assert codes == {BAD_MATRIX, BAD_RES1, BAD_RES2, UNSUPPORTED}


def test_a_bad_residue_or_1025_residues_in_a_cluster_of_one_raise_nothing_of_their_own(lib):
    import dynaalign_amd as da
    rows = [("ACD", 1), ("A?D", "one"), ("ACE", 1), ("A" * 1025, "long")]
    if lib.da_device_count() > 0:
        assert da.clusterconsensus_device(rows) == da.clusterconsensus(rows)
        return
    for fn in (da.clusterconsensus_device, da.clusterconsensus):
        with pytest.raises(da.DynaAlignError) as e:
            fn(rows)
        assert e.value.code == NO_DEVICE and "no CPU fallback" in str(e.value)


def raw(lib, seqs, cluster_of, clusters, matrix=b"BLOSUM62", ld=None, nulls=()):
    import oracle_lib as O
    res, off = O.pack(seqs)
    cl = np.ascontiguousarray(cluster_of, np.int32)
    ld = max([len(s) for s in seqs] + [1]) if ld is None else ld
    cons = np.full((max(clusters, 1), max(ld, 1)), 7, np.uint8)
    ln = np.full(max(clusters, 1), -7, np.int32)
    cen = np.full(max(clusters, 1), -7, np.int32)
    args = {"res": res.ctypes.data, "off": off.ctypes.data, "cl": cl.ctypes.data, "cons": cons.ctypes.data, "ln": ln.ctypes.data}
    for k in nulls:
        args[k] = None
    rc = lib.da_cluster_consensus(args["res"], args["off"], len(seqs), args["cl"], clusters, matrix, 10, 4, args["cons"], ld, args["ln"],
                                  cen.ctypes.data)
    untouched = bool((cons == 7).all() and (ln == -7).all() and (cen == -7).all())
    return rc, (lib.da_last_error().decode("latin-1") if rc else ""), untouched, (cons, ln, cen)


def test_c_boundary_validation_order(lib):
    seqs = ["ACD", "A?D", "ACE"]
    assert raw(lib, seqs, [0, 0, 5], 1, matrix=b"nope")[:3] == (BAD_MATRIX, "Invalid substitution matrix name: nope", True)
    for null in ("res", "cl", "cons", "ln", "off"):
        rc, msg, untouched, _ = raw(lib, seqs, [0, 0, 5], 1, nulls=(null,))
        assert rc == BAD_ARG and untouched, null
    rc, msg, untouched, _ = raw(lib, seqs, [0, 0, 5], 3)                 # the range of cluster_of comes before the residues
    assert rc == BAD_ARG and "outside" in msg and untouched
    rc, msg, untouched, _ = raw(lib, seqs, [0, 0, 2], 3)                 # ... and so does a cluster without a member
    assert rc == BAD_ARG and "cluster 1 has no member" in msg and untouched
    rc, msg, untouched, _ = raw(lib, ["A" * 1025, "?", "ACD"], [0, 0, 1], 2, ld=1)   # the length before ld_cons and the residues
    assert rc == UNSUPPORTED and "1024" in msg and untouched
    rc, msg, untouched, _ = raw(lib, ["ACDE", "?", "ACD"], [0, 0, 1], 2, ld=3)       # ld_cons before the residues
    assert rc == BAD_ARG and "ld_cons = 3" in msg and untouched
    rc, msg, untouched, _ = raw(lib, ["ACDE", "?", "ACD"], [0, 0, 1], 2)
    assert rc == BAD_RES2 and msg == "Invalid amino acid in sequence2: ?" and untouched
    assert raw(lib, [], [], 0)[0] == OK


def test_c_boundary_copies_clusters_of_one_through(lib):
    rc, msg, untouched, (cons, ln, cen) = raw(lib, ["ACD", "W?", ""], [2, 0, 1], 3)
    assert rc == OK and ln.tolist() == [2, 0, 3] and cen.tolist() == [1, 2, 0]
    assert bytes(cons[0][:2]) == b"W?" and bytes(cons[2][:3]) == b"ACD" and not cons[0][2:].any() and not cons[1].any()
    if lib.da_device_count() == 0:                                       # two members: valid input fails loudly, nothing written
        rc, msg, untouched, _ = raw(lib, ["ACD", "ACE", "WW"], [0, 0, 1], 2)
        assert rc == NO_DEVICE and untouched and "no CPU fallback" in msg


def test_workspace_bytes_need_no_device(lib):
    from dynaalign_amd import device
    ptr = [0, 3, 4, 70]
    small, full = device.cluster_consensus_workspace_bytes(ptr, 20, minimal=True), device.cluster_consensus_workspace_bytes(ptr, 20)
    assert 0 < small < full
    # phase 1 of this table has 3 * 2 + 66 * 65 pairs, phase 2 has 67 rows: 5 KiB of decisions a pair and 40 bytes of ops a row
    assert full >= (6 + 66 * 65) * 5120 and small < 64 * (5120 + 16 + 40) + 70 * 16 + 4096
    assert device.cluster_consensus_workspace_bytes(ptr, 200, minimal=True) > 0
    assert lib.da_dev_cluster_consensus_workspace_bytes(None, 3, 20, 0) == 0
