"""CPU tests of what device.py refuses before it calls the library: the exception class and the text of every refusal are part of its
contract.  No device call is made here.  A host tensor is refused by every public function that checks where its operands live; the
functions that do not check (nw, nw_rect, cluster_consensus, symmetrize, widen, the histogram and edge extraction helpers, edges_to_csr,
the plan consumers) would hand a host pointer to a kernel and are not called.  The refusals behind that first check are reached with host
tensors that claim to live in HBM: they raise before anything is launched."""
import numpy as np
import pytest
import torch

from dynaalign_amd import _capi, device

NO_CPU = "%s must live in HBM (dynaalign_amd has no CPU path)"


class _Resident(torch.Tensor):
    """a host tensor that says it lives in HBM: passes _require_cuda and nothing else"""
    is_cuda = True


def resident(t):
    return t.as_subclass(_Resident)


def host_set(encoded=False):
    ds = device.DeviceSequences(np.frombuffer(b"ACDEFGHIKLMNPQRS", np.uint8), np.array([0, 8, 16]), device="cpu")
    if encoded:
        ds.codes = torch.zeros(16, dtype=torch.uint8)
    return ds


def i16(*shape):
    return torch.zeros(shape, dtype=torch.int16)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


SEEDS = np.arange(8, dtype=np.uint32)
SETS = device.JaccardSets(i32(2, 8), u8(2), 2, 4)
SETS_LONG = device.JaccardSets(i32(2, 8), i16(2), 2, 4)
SIG = i32(2, 32)

HOST_TENSOR_CALLS = {
    "minhash_signatures": ("residues", lambda: device.minhash_signatures(host_set(), 4, 8, SEEDS)),
    "mh_planes": ("signatures", lambda: device.mh_planes(SIG, 2, 8)),
    "mh_compare": ("bit planes", lambda: device.mh_compare(device.Planes(i32(64), 32), 2, 8)),
    "mh_compare_rect": ("bit planes", lambda: device.mh_compare_rect(device.Planes(i32(64), 32), 2, 8, 0, 1, 1, 2)),
    "nw_encode": ("residues", lambda: device.nw_encode(host_set())),
    "jaccard_sets": ("residues", lambda: device.jaccard_sets(host_set(), 4)),
    "jaccard_rect": ("shingle sets", lambda: device.jaccard_rect(SETS)),
    "jaccard_sets_long": ("residues", lambda: device.jaccard_sets_long(host_set(), 4)),
    "jaccard_rect_long": ("shingle sets", lambda: device.jaccard_rect_long(SETS_LONG)),
    "nw_align_pairs": ("pair_x", lambda: device.nw_align_pairs(host_set(True), host_set(True), pair_x=i32(2), pair_y=i32(2))),
    "nw_align_long_pairs": ("pair_x", lambda: device.nw_align_long_pairs(host_set(True), host_set(True), pair_x=i32(2), pair_y=i32(2))),
    "consensus_center_sums": ("length", lambda: device.consensus_center_sums(i32(2), i32(2), [0, 2])),
    "consensus_pick": ("sums", lambda: device.consensus_pick(i64(2, 2), [0, 2])),
    "consensus_vote": ("ops", lambda: device.consensus_vote(host_set(True), [0, 2], i32(1), u8(1, 16))),
    "louvain_csr": ("ptr", lambda: device.louvain_csr(i64(3), i32(2), i16(2), None, [1.0])),
    "components_edges": ("ei", lambda: device.components_edges(i32(2), i32(2), 2)),
    "components_csr": ("ptr", lambda: device.components_csr(i64(3), i32(2))),
    "similarity_mh": ("residues", lambda: device.similarity_mh(host_set(), 4, 8, SEEDS)),
    "similarity_mh_cross": ("residues of x", lambda: device.similarity_mh_cross(host_set(), host_set(), 4, 8, SEEDS)),
    "topk_rows": ("keys", lambda: device.topk_rows(i16(2, 8), 2)),
    "topk_ranks": ("keys", lambda: device.topk_ranks(i32(2, 8), 2, 16)),
    "similarity_mh_knn": ("residues", lambda: device.similarity_mh_knn(host_set(), 4, 8, SEEDS, 1)),
    "knn_edges": ("idx", lambda: device.knn_edges(i32(2, 1), i16(2, 1))),
    "similarity_mh_cross_topk": ("residues of x", lambda: device.similarity_mh_cross_topk(host_set(), host_set(), 4, 8, SEEDS, 1)),
    "rect_histogram": ("keys", lambda: device.rect_histogram(i16(2, 8), 9)),
    "threshold_rows": ("keys", lambda: device.threshold_rows(i16(2, 8), np.ones(9, np.uint8))),
    "nw_codes_to_ranks": ("keys", lambda: device.nw_codes_to_ranks(i32(2, 8), i32(15), 2)),
    "rank_histogram": ("keys", lambda: device.rank_histogram(i32(2, 8), 9)),
    "threshold_ranks": ("keys", lambda: device.threshold_ranks(i32(2, 8), 1, 9)),
    "upper_extrema": ("keys", lambda: device.upper_extrema(i16(2, 8), 8)),
    "similarity_mh_cross_edges": ("residues of x", lambda: device.similarity_mh_cross_edges(host_set(), host_set(), 4, 8, SEEDS, threshold=0.5)),
    "lsh_band_keys": ("signatures", lambda: device.lsh_band_keys(SIG, 8, 2, 4)),
    "lsh_verify_pairs": ("signatures", lambda: device.lsh_verify_pairs(SIG, 8, 2, 4, 0.5, [0], [1], [0])),
    "lsh_edges": ("signatures", lambda: device.lsh_edges(SIG, 8, 2, 4, 0.5)),
    "lsh_components": ("signatures", lambda: device.lsh_components(SIG, 8, 2, 4, 0.5)),
    "lsh_knn_select": ("ptr", lambda: device.lsh_knn_select(i64(3), i32(2), i16(2), 1)),
    "lsh_knn": ("signatures", lambda: device.lsh_knn(SIG, 8, 2, 4, 1)),
    "lsh_index_build": ("signatures", lambda: device.lsh_index_build(SIG, 8, 2, 4)),
    "lsh_index_probe": ("signatures", lambda: device.lsh_index_probe(u8(4096), 2, SIG, 8, 2, 4)),
    "lsh_cross_verify_pairs": ("signatures", lambda: device.lsh_cross_verify_pairs(SIG, SIG, 8, 2, 4, 0.5, [0], [1], [0])),
    "lsh_cross_edges": ("signatures", lambda: device.lsh_cross_edges(u8(4096), SIG, SIG, 8, 2, 4, 0.5)),
    "lsh_cross_topk": ("signatures", lambda: device.lsh_cross_topk(u8(4096), SIG, SIG, 8, 2, 4, 1)),
    "nw_rescore_pairs": ("i", lambda: device.nw_rescore_pairs(host_set(True), host_set(True), i32(2), i32(2))),
    "lsh_nw_edges": ("signatures", lambda: device.lsh_nw_edges(SIG, host_set(True), 8, 2, 4, 0.5)),
    "lsh_nw_edges, two sets": ("signatures", lambda: device.lsh_nw_edges(SIG, host_set(True), 8, 2, 4, 0.5, index=u8(4096), sig_y=SIG,
                                                                         dy=host_set(True))),
    "UniquePlan": ("sequence bytes", lambda: device.UniquePlan(u8(16), i64(3), 2, 16)),
}


@pytest.mark.parametrize("name", sorted(HOST_TENSOR_CALLS))
def test_a_host_tensor_is_refused(built, name):
    what, call = HOST_TENSOR_CALLS[name]
    with pytest.raises(_capi.DynaAlignError) as e:
        call()
    assert (e.value.code, str(e.value)) == (_capi.DA_ERR_NO_DEVICE, NO_CPU % what)


def test_the_second_operand_is_checked_too(built):
    """where two operands are checked, the first one in HBM does not excuse the second"""
    with pytest.raises(_capi.DynaAlignError) as e:
        device.knn_edges(resident(i32(2, 1)), i16(2, 1))
    assert str(e.value) == NO_CPU % "key"
    with pytest.raises(_capi.DynaAlignError) as e:
        device.topk_rows(resident(i16(2, 8)), 2, rank=i16(65536), rank_bits=16)
    assert str(e.value) == NO_CPU % "rank table"
    for fn in (device.lsh_edges, device.lsh_knn):
        with pytest.raises(_capi.DynaAlignError) as e:
            fn(resident(SIG), 8, 2, 4, 1, work=u8(64))
        assert str(e.value) == NO_CPU % "work"


@pytest.mark.parametrize("fn, keys, args", [(device.topk_rows, i16(2, 8), (2,)), (device.topk_ranks, i32(2, 8), (2, 16))],
                         ids=["topk_rows", "topk_ranks"])
def test_want_self_needs_self_col0(built, fn, keys, args):
    with pytest.raises(ValueError) as e:
        fn(resident(keys), *args, want_self=True)
    assert type(e.value) is ValueError and str(e.value) == "want_self needs self_col0"


def test_knn_edges_refuses_an_unknown_mode(built):
    with pytest.raises(ValueError) as e:
        device.knn_edges(resident(i32(2, 1)), resident(i16(2, 1)), mode="x")
    assert type(e.value) is ValueError and str(e.value) == "mode must be 'union' or 'mutual'"


def test_lsh_nw_edges_two_set_form_needs_all_three(built):
    for kw in ({}, {"sig_y": SIG}, {"dy": host_set(True)}):
        with pytest.raises(ValueError) as e:
            device.lsh_nw_edges(SIG, host_set(True), 8, 2, 4, 0.5, index=u8(4096), **kw)
        assert type(e.value) is ValueError and str(e.value) == "the two-set form needs index, sig_y and dy"
    with pytest.raises(ValueError) as e:
        device.lsh_nw_edges(SIG, host_set(), 8, 2, 4, 0.5)
    assert str(e.value) == "call nw_encode on the sequences first"


def test_lsh_verify_pairs_refuses_unequal_lengths(built):
    with pytest.raises(ValueError) as e:
        device.lsh_verify_pairs(resident(SIG), 8, 2, 4, 0.5, [0, 1], [1], [0, 0])
    assert type(e.value) is ValueError and str(e.value) == "i, j and band must have the same number of entries"
    with pytest.raises(ValueError) as e:
        device.lsh_cross_verify_pairs(resident(SIG), resident(SIG), 8, 2, 4, 0.5, [0], [1], [0, 0])
    assert str(e.value) == "i, j and band must have the same number of entries"


def test_buffer_refusals_keep_their_class_and_text(built):
    """the byte buffers: ValueError from the LSH functions, DynaAlignError (DA_ERR_BAD_ARG) from the components family, and the shape of
    the signatures"""
    sig = resident(SIG)
    with pytest.raises(ValueError) as e:
        device.lsh_edges(resident(i32(2, 4)), 8, 2, 4, 0.5)
    assert str(e.value) == "signatures must be a 2-d tensor of 32-bit words with unit column stride and at least n_hash columns"
    for fn in (device.lsh_edges, device.lsh_knn):
        for work in (resident(i32(64)), resident(u8(128)[::2])):
            with pytest.raises(ValueError) as e:
                fn(sig, 8, 2, 4, 1, work=work)
            assert type(e.value) is ValueError
            assert str(e.value) == "work must be a contiguous uint8 tensor of lsh_workspace_bytes(n, bands) bytes"
    with pytest.raises(ValueError) as e:
        device.lsh_index_build(sig, 8, 2, 4, out=resident(i32(64)))
    assert str(e.value) == "out must be a contiguous uint8 tensor of lsh_index_bytes(n, bands) bytes"
    with pytest.raises(ValueError) as e:
        device.lsh_cross_edges(resident(u8(128)[::2]), sig, sig, 8, 2, 4, 0.5)
    assert str(e.value) == "index must be a contiguous uint8 tensor of lsh_index_bytes(n, bands) bytes"
    with pytest.raises(ValueError) as e:
        device.lsh_cross_topk(resident(u8(4096)), sig, sig, 8, 2, 4, 1, work=resident(i32(64)))
    assert str(e.value) == "work must be a contiguous uint8 tensor of lsh_cross_workspace_bytes(m, bands) bytes"
    with pytest.raises(ValueError) as e:
        device.lsh_nw_edges(sig, host_set(True), 8, 2, 4, 0.5, work=resident(i32(64)))
    assert str(e.value) == "work must be a contiguous uint8 tensor of lsh_workspace_bytes(n, bands) bytes"
    for work in (resident(i32(64)), resident(u8(128)[::2]), resident(u8(8, 8))):
        with pytest.raises(ValueError) as e:
            device.nw_rescore_pairs(host_set(True), host_set(True), resident(i32(2)), resident(i32(2)), work=work)
        assert type(e.value) is ValueError and str(e.value) == "work must be a 1-d uint8 tensor with unit stride"
    ei = resident(i32(2))
    for work in (resident(i32(1 << 16)), resident(u8(1 << 17)[::2]), resident(u8(8))):
        with pytest.raises(_capi.DynaAlignError) as e:
            device.components_edges(ei, ei, 2, work=work)
        assert (e.value.code, str(e.value)) == (_capi.DA_ERR_BAD_ARG, "work must be a contiguous uint8 tensor of components_workspace_bytes(n) bytes")
        with pytest.raises(_capi.DynaAlignError) as e:
            device.lsh_components(sig, 8, 2, 4, 0.5, work=work)
        assert (e.value.code, str(e.value)) == (
            _capi.DA_ERR_BAD_ARG, "work must be a contiguous uint8 tensor of lsh_workspace_bytes(n, bands) + components_workspace_bytes(n) bytes")
    with pytest.raises(_capi.DynaAlignError) as e:
        device.components_edges(ei, ei, 2, work=u8(1 << 16))
    assert (e.value.code, str(e.value)) == (_capi.DA_ERR_NO_DEVICE, NO_CPU % "work")
