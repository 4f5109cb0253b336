"""GPU tests of the marshalling contract of device.py, whatever the kernels compute: the capacity protocol of the list functions, the
handling of a caller's workspace, seeds as a numpy array or as a device tensor, the result arity and selection of the top-k pair, and
empty blocks.  Results are compared with each other or with numpy, element for element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 12345
K, N_HASH, BANDS, ROWS = 3, 16, 4, 4
MH_THRESHOLD, NW_THRESHOLD = 0.5, 0.5
WORK_TEXT = "work must be a contiguous uint8 tensor of %s bytes"


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def peptides():
    """70 peptides of 12 .. 20 residues; the last ten are copies of the first ten, five exact and five with one residue replaced"""
    from dynaalign_amd import synth
    res, off = synth.uniform_peptides(70, 20, seed=31)
    seqs = [s[:12 + i % 9] for i, s in enumerate(synth.to_strings(res, off))]
    for t in range(5):
        seqs[60 + t] = seqs[t]
        src = seqs[5 + t]
        seqs[65 + t] = src[:6] + ("W" if src[6] != "W" else "Y") + src[7:]
    assert len(seqs) == 70 and all(12 <= len(s) <= 20 for s in seqs) and len(set(seqs)) == 65
    return seqs


class Case:
    """the resident sets: all 70 sequences, and the overlapping halves x = [0, 50) and y = [20, 70) of the two-set calls"""

    def __init__(self, da):
        from dynaalign_amd import device
        self.seqs = peptides()
        self.seeds = da.hash_family_seeds(SEED, N_HASH)
        assert self.seeds.dtype == np.uint32 and (self.seeds >= 2 ** 31).any()      # the int32 view has negative words
        self.ds, self.dx, self.dy = (self.resident(s) for s in (self.seqs, self.seqs[:50], self.seqs[20:]))
        self.sig, self.sig_x, self.sig_y = (device.minhash_signatures(d, K, N_HASH, self.seeds, want_planes=False)[0][:d.n]
                                            for d in (self.ds, self.dx, self.dy))
        self.index = device.lsh_index_build(self.sig_y, N_HASH, BANDS, ROWS)

    @staticmethod
    def resident(seqs):
        from dynaalign_amd import device
        import dynaalign_amd
        ds = device.DeviceSequences(*dynaalign_amd.pack_sequences(seqs))
        assert int(device.nw_encode(ds).item()) == 0
        return ds


@pytest.fixture(scope="module")
def case(da):
    return Case(da)


def block(dtype, rows=5, seed=3):
    """a (rows, 37) view with row stride 40 that starts one element into its storage: an unaligned base and a tail shorter than one 16-byte
    load; keys in 0 .. 299 so that rows hold ties"""
    store = torch.from_numpy(np.random.RandomState(seed).randint(0, 300, 1 + 5 * 40).astype(np.int64)).to("cuda").to(dtype)
    view = torch.as_strided(store, (rows, 37), (40, 1), 1)
    assert rows == 0 or view.data_ptr() % 16 == store.element_size()       # (torch gives a view without elements the address 0)
    return view


def as_numpy(result):
    return [np.ascontiguousarray(x.cpu().numpy()) if torch.is_tensor(x) else np.asarray(x) for x in result]


def identical(a, b):
    a, b = as_numpy(a), as_numpy(b)
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ---- the capacity protocol ------------------------------------------------------------------------------------------------------------------
def list_calls(case):
    """name -> call(capacity) -> (the list tensors, the full count the call reports, what else it returns)"""
    from dynaalign_amd import device
    keep = (np.arange(300) % 2).astype(np.uint8)

    def lsh(capacity):
        r = device.lsh_edges(case.sig, N_HASH, BANDS, ROWS, MH_THRESHOLD, capacity=capacity)
        return r, device.mh_lsh_last_route()["edges"], ()

    def lsh_cross(capacity):
        r = device.lsh_cross_edges(case.index, case.sig_x, case.sig_y, N_HASH, BANDS, ROWS, MH_THRESHOLD, capacity=capacity)
        return r, device.mh_lsh_last_route()["edges"], ()

    def lsh_nw(capacity):
        r = device.lsh_nw_edges(case.sig, case.ds, N_HASH, BANDS, ROWS, NW_THRESHOLD, capacity=capacity)
        return r, device.nw_lsh_last_route()["edges"], ()

    def lsh_nw_cross(capacity):
        r = device.lsh_nw_edges(case.sig_x, case.dx, N_HASH, BANDS, ROWS, NW_THRESHOLD, capacity=capacity, index=case.index, sig_y=case.sig_y,
                                dy=case.dy)
        return r, device.nw_lsh_last_route()["edges"], ()

    def rows16(capacity):
        rowptr, j, key = device.threshold_rows(block(torch.int16), keep, capacity=capacity)
        return (j, key), int(rowptr[-1].item()), (rowptr,)

    def ranks32(capacity):
        rowptr, j, key = device.threshold_ranks(block(torch.int32), 150, 300, capacity=capacity)
        return (j, key), int(rowptr[-1].item()), (rowptr,)

    def mh_cross(capacity):
        thr, rowptr, j, w = device.similarity_mh_cross_edges(case.dx, case.dy, K, N_HASH, case.seeds, threshold=1.0 / N_HASH, capacity=capacity)
        return (j, w), int(rowptr[-1].item()), (rowptr, thr)

    return {"lsh_edges": lsh, "lsh_cross_edges": lsh_cross, "lsh_nw_edges": lsh_nw, "lsh_nw_edges, two sets": lsh_nw_cross,
            "threshold_rows": rows16, "threshold_ranks": ranks32, "similarity_mh_cross_edges": mh_cross}


LIST_CALLS = ["lsh_edges", "lsh_cross_edges", "lsh_nw_edges", "lsh_nw_edges, two sets", "threshold_rows", "threshold_ranks",
              "similarity_mh_cross_edges"]


@pytest.mark.parametrize("name", LIST_CALLS)
def test_capacity_protocol(case, name):
    call = list_calls(case)[name]
    whole, count, rest = call(None)
    assert count >= 10 and all(t.dim() == 1 and t.numel() == count for t in whole)
    exact, count_exact, rest_exact = call(count)
    assert count_exact == count and identical(exact, whole) and identical(rest_exact, rest)
    part, count_part, rest_part = call(count - 3)
    assert count_part == count and identical(part, [t[:count - 3] for t in whole]) and identical(rest_part, rest)
    none, count_none, rest_none = call(0)
    assert count_none == count and identical(none, [t[:0] for t in whole]) and identical(rest_none, rest)


@pytest.mark.parametrize("name", LIST_CALLS)
def test_library_calls_and_read_backs_per_call(case, name, monkeypatch):
    """capacity=None is a counting call and a filling call in the LSH functions, count + emit with ONE read-back of rowptr[rows] in the
    threshold functions, and one call when the first guess holds the list; a capacity is one call (count + emit: two) and no read-back"""
    from dynaalign_amd import device
    calls, items = [], []
    real_call, real_item = device._call, torch.Tensor.item

    def counting_call(fn, *args):
        calls.append(fn)
        return real_call(fn, *args)

    def counting_item(self):
        items.append(self)
        return real_item(self)

    def run(capacity):
        with monkeypatch.context() as m:
            m.setattr(device, "_call", counting_call)
            del calls[:], items[:]
            args = (block(torch.int16), (np.arange(300) % 2).astype(np.uint8)) if name == "threshold_rows" else (block(torch.int32), 150, 300)
            if name.startswith("threshold"):
                m.setattr(torch.Tensor, "item", counting_item)
                getattr(device, name)(*args, capacity=capacity)
            else:
                list_calls(case)[name](capacity)
        return len(calls), len(items)

    count = list_calls(case)[name](None)[1]
    if name.startswith("threshold"):
        assert run(None) == (2, 1) and run(count) == (2, 0) and run(0) == (1, 0)
    elif name == "similarity_mh_cross_edges":
        assert run(None)[0] == 1 and run(count)[0] == 1 and run(0)[0] == 1
    else:
        assert run(None)[0] == 2 and run(count)[0] == 1 and run(0)[0] == 1


# ---- a caller's workspace -------------------------------------------------------------------------------------------------------------------
def work_calls(case):
    """name -> (call(work), bytes of the documented size, the refusal of a wrong dtype / a non-contiguous view: (class, code, text))"""
    from dynaalign_amd import _capi, device
    n, m = case.ds.n, case.dx.n
    ei, ej, ec = device.lsh_edges(case.sig, N_HASH, BANDS, ROWS, MH_THRESHOLD)
    ptr, adj, _, _ = device.edges_to_csr(ei, ej, ec, ei.numel(), n)
    lsh_bytes, cc_bytes = device.lsh_workspace_bytes(n, BANDS), device.components_workspace_bytes(n)
    value_error = lambda what: (ValueError, None, WORK_TEXT % what)
    bad_arg = lambda what: (_capi.DynaAlignError, _capi.DA_ERR_BAD_ARG, WORK_TEXT % what)
    return {
        "lsh_edges": (lambda w: device.lsh_edges(case.sig, N_HASH, BANDS, ROWS, MH_THRESHOLD, work=w), lsh_bytes,
                      value_error("lsh_workspace_bytes(n, bands)")),
        "lsh_knn": (lambda w: device.lsh_knn(case.sig, N_HASH, BANDS, ROWS, 5, work=w), lsh_bytes, value_error("lsh_workspace_bytes(n, bands)")),
        "lsh_components": (lambda w: device.lsh_components(case.sig, N_HASH, BANDS, ROWS, MH_THRESHOLD, sizes=True, work=w), lsh_bytes + cc_bytes,
                           bad_arg("lsh_workspace_bytes(n, bands) + components_workspace_bytes(n)")),
        "components_edges": (lambda w: device.components_edges(ei, ej, n, sizes=True, work=w), cc_bytes, bad_arg("components_workspace_bytes(n)")),
        "components_csr": (lambda w: device.components_csr(ptr, adj, sizes=True, work=w), cc_bytes, bad_arg("components_workspace_bytes(n)")),
        "lsh_cross_edges": (lambda w: device.lsh_cross_edges(case.index, case.sig_x, case.sig_y, N_HASH, BANDS, ROWS, MH_THRESHOLD, work=w),
                            device.lsh_cross_workspace_bytes(m, BANDS), value_error("lsh_cross_workspace_bytes(m, bands)")),
        "lsh_nw_edges": (lambda w: device.lsh_nw_edges(case.sig, case.ds, N_HASH, BANDS, ROWS, NW_THRESHOLD, work=w), lsh_bytes,
                         value_error("lsh_workspace_bytes(n, bands)")),
        "lsh_nw_edges, two sets": (lambda w: device.lsh_nw_edges(case.sig_x, case.dx, N_HASH, BANDS, ROWS, NW_THRESHOLD, work=w, index=case.index,
                                                                 sig_y=case.sig_y, dy=case.dy),
                                   device.lsh_cross_workspace_bytes(m, BANDS), value_error("lsh_cross_workspace_bytes(m, bands)")),
        "nw_rescore_pairs": (lambda w: device.nw_rescore_pairs(case.ds, case.ds, ei, ej, work=w), device.nw_rescore_workspace_bytes(ei.numel()),
                             (ValueError, None, "work must be a 1-d uint8 tensor with unit stride")),
    }


WORK_CALLS = ["lsh_edges", "lsh_knn", "lsh_components", "components_edges", "components_csr", "lsh_cross_edges", "lsh_nw_edges",
              "lsh_nw_edges, two sets", "nw_rescore_pairs"]


@pytest.mark.parametrize("name", WORK_CALLS)
def test_work_none_and_a_callers_buffer(case, name):
    from dynaalign_amd import _capi
    call, nbytes, (cls, code, text) = work_calls(case)[name]
    assert nbytes > 0
    want = call(None)
    assert identical(call(torch.empty(nbytes, dtype=torch.uint8, device="cuda")), want)
    for work in (torch.empty(nbytes, dtype=torch.int32, device="cuda"), torch.empty(2 * nbytes, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(cls) as e:
            call(work)
        assert type(e.value) is cls and str(e.value) == text and getattr(e.value, "code", None) == code
    with pytest.raises(_capi.DynaAlignError) as e:
        call(torch.empty(nbytes, dtype=torch.uint8))
    assert (e.value.code, str(e.value)) == (_capi.DA_ERR_NO_DEVICE, "work must live in HBM (dynaalign_amd has no CPU path)")
    if cls is _capi.DynaAlignError:                            # the components family sizes its buffer on this side
        with pytest.raises(cls) as e:
            call(torch.empty(nbytes - 1, dtype=torch.uint8, device="cuda"))
        assert (e.value.code, str(e.value)) == (code, text)
    assert identical(call(None), want)


# ---- seeds ----------------------------------------------------------------------------------------------------------------------------------
SEED_CALLS = {
    "minhash_signatures": lambda d, c, s: (d.minhash_signatures(c.ds, K, N_HASH, s, want_planes=False)[0][:c.ds.n, :N_HASH],),
    "similarity_mh": lambda d, c, s: (d.similarity_mh(c.ds, K, N_HASH, s),),
    "similarity_mh_cross": lambda d, c, s: (d.similarity_mh_cross(c.dx, c.dy, K, N_HASH, s),),
    "similarity_mh_knn": lambda d, c, s: d.similarity_mh_knn(c.ds, K, N_HASH, s, 5),
    "similarity_mh_cross_topk": lambda d, c, s: d.similarity_mh_cross_topk(c.dx, c.dy, K, N_HASH, s, 5),
    "similarity_mh_cross_edges": lambda d, c, s: d.similarity_mh_cross_edges(c.dx, c.dy, K, N_HASH, s, threshold=1.0 / N_HASH),
}


@pytest.mark.parametrize("name", sorted(SEED_CALLS))
def test_seeds_as_numpy_uint32_or_device_int32(case, name):
    from dynaalign_amd import device
    on_device = torch.from_numpy(case.seeds.view(np.int32).copy()).to("cuda")
    a, b = SEED_CALLS[name](device, case, case.seeds), SEED_CALLS[name](device, case, on_device)
    a, b = [[x.view(np.uint8) if x.ndim else x for x in as_numpy(r)] for r in (a, b)]           # bit patterns, not values
    assert identical(a, b) and sum(x.size for x in a) > 0
    if name == "minhash_signatures":
        assert identical([a[0]], [np.ascontiguousarray(case.sig[:, :N_HASH].cpu().numpy()).view(np.uint8)])


# ---- the top-k pair -------------------------------------------------------------------------------------------------------------------------
def topk_model(keys, top, self_col0=None):
    idx = []
    for r, row in enumerate(keys.astype(np.int64)):
        order = np.argsort(-row, kind="stable")
        idx.append((order if self_col0 is None else order[order != self_col0 + r])[:top])
    idx = np.array(idx, np.int32).reshape(len(keys), top)
    return idx, np.take_along_axis(keys, idx.astype(np.int64), axis=1)


@pytest.mark.parametrize("name, dtype, extra", [("topk_rows", torch.int16, ()), ("topk_ranks", torch.int32, (300,))], ids=["rows", "ranks"])
def test_topk_results(da, name, dtype, extra):
    from dynaalign_amd import device
    fn, keys = getattr(device, name), block(dtype)
    host = keys.cpu().numpy()
    assert keys.shape == (5, 37) and keys.stride() == (40, 1) and any(len(set(row)) < 37 for row in host.tolist())
    got = fn(keys, 5, *extra)
    assert len(got) == 2 and got[0].dtype == torch.int32 and got[1].dtype == dtype and identical(got, topk_model(host, 5))
    got = fn(keys, 5, *extra, self_col0=30)
    assert len(got) == 2 and identical(got, topk_model(host, 5, 30))
    got = fn(keys, 5, *extra, self_col0=30, want_self=True)
    assert len(got) == 3 and identical(got[:2], topk_model(host, 5, 30))
    assert got[2].dtype == dtype and np.array_equal(got[2].cpu().numpy(), host[np.arange(5), 30 + np.arange(5)])
    with pytest.raises(ValueError) as e:
        fn(keys, 5, *extra, want_self=True)
    assert str(e.value) == "want_self needs self_col0"


@pytest.mark.parametrize("name, dtype, extra", [("topk_rows", torch.int16, ()), ("topk_ranks", torch.int32, (300,))], ids=["rows", "ranks"])
def test_topk_of_an_empty_block(da, name, dtype, extra):
    """a (0, 37) block gives (0, 5) tensors, whichever form is asked for.  torch reports the address 0 for a view without elements and
    da_dev_topk_ranks refuses a NULL block before it looks at the row count, so such a block must not reach the library."""
    from dynaalign_amd import device
    fn, empty = getattr(device, name), block(dtype, rows=0)
    assert empty.shape == (0, 37)
    for kw, arity in (({}, 2), ({"self_col0": 0}, 2), ({"self_col0": 0, "want_self": True}, 3)):
        got = fn(empty, 5, *extra, **kw)
        assert len(got) == arity and got[0].shape == (0, 5) and got[1].shape == (0, 5) and (got[0].dtype, got[1].dtype) == (torch.int32, dtype)
        assert arity == 2 or (got[2].shape == (0,) and got[2].dtype == dtype)


# ---- empty blocks ---------------------------------------------------------------------------------------------------------------------------
def test_threshold_functions_on_an_empty_block(da):
    from dynaalign_amd import device
    for got, dtype in ((device.threshold_rows(block(torch.int16, rows=0), np.ones(300, np.uint8)), torch.int16),
                       (device.threshold_ranks(block(torch.int32, rows=0), 0, 300), torch.int32)):
        rowptr, j, key = got
        assert rowptr.dtype == torch.int64 and rowptr.tolist() == [0]
        assert j.dtype == torch.int32 and key.dtype == dtype and j.numel() == 0
    rowptr, j, key = device.threshold_ranks(block(torch.int32, rows=0), 0, 300, capacity=4)     # the slots asked for, nothing in them
    assert rowptr.tolist() == [0] and j.shape == (4,) and key.shape == (4,)
