"""GPU tests of the one-set nearest-neighbour forms: the selection kernel with a row's own column excluded (device.topk_rows with
self_col0) against numpy on the keys, similarityMH_knn / similarityNW_knn through every entry point against the CPU oracle's dense matrix
(knn_dense), row blocks, and the lists -> edge list kernel (device.knn_edges) against knn_graph.  Every comparison is exact: indices as
integers, values as uint64 bit patterns."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_cross import SEED, bits, strided, switches, two_sets
from test_gpu_topk import nw_sets

pytestmark = pytest.mark.gpu

ALPHABET = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def da(built):
    import dynaalign_amd
    from dynaalign_amd import _capi
    assert _capi.load().da_device_count() > 0
    return dynaalign_amd


def assert_lists(got, S, top, what):
    from dynaalign_amd import knn_dense
    idx, val = got
    want_idx, want_val = knn_dense(S, top)
    idx = np.asarray(idx)
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape, (what, idx.dtype, idx.shape, want_idx.shape)
    bad = np.argwhere(idx != want_idx)
    assert len(bad) == 0, (what, "first index difference at", bad[0].tolist(), idx[bad[0][0]][:12], want_idx[bad[0][0]][:12])
    if val is not None:
        val = np.asarray(val)
        assert val.dtype == np.float64 and np.array_equal(bits(val), bits(want_val)), (what, "values differ")


# ---- the selection kernel alone ------------------------------------------------------------------------------------------------------------

ROWS = 6


def self_block(rng, n, col0, hi, own_max):
    """ROWS rows of n keys for a block whose row r owns column col0 + r: a repeated key, all zero, the own element the unique maximum, the
    own element among the ties at the rank of the top-th element (5s on both sides of it, three 9s above), random with heavy ties and many
    zeros, increasing"""
    keys = rng.randint(0, hi, (ROWS, n)).astype(np.uint16)
    keys[rng.rand(ROWS, n) < 0.5] = 0
    keys[0] = 123 % hi
    keys[1] = 0
    if 0 <= col0 + 2 < n:
        keys[2, col0 + 2] = own_max
    keys[3] = 5
    for c in rng.randint(0, n, 3):
        if c != col0 + 3:
            keys[3, c] = 9
    keys[4] = rng.randint(0, 4, n)
    keys[5] = (np.arange(n) % hi).astype(np.uint16)
    return keys


def run_self(keys, top, ld, offset, col0, rank=None, rank_bits=0):
    from dynaalign_amd import device
    rows, n = keys.shape
    buf, view = strided(rows, n, ld, torch.int16, offset)
    view.copy_(torch.from_numpy(keys.view(np.int16)).cuda())
    rank_t = None if rank is None else torch.from_numpy(np.ascontiguousarray(rank, np.uint16).view(np.int16)).cuda()
    idx, key, own = device.topk_rows(view, top, rank_t, rank_bits, self_col0=col0, want_self=True)
    torch.cuda.synchronize()
    idx, key, own = idx.cpu().numpy(), key.cpu().numpy().view(np.uint16), own.cpu().numpy().view(np.uint16)
    r = (keys if rank is None else rank[keys]).astype(np.int64)
    cols = col0 + np.arange(rows)
    has = (cols >= 0) & (cols < n)
    r[np.nonzero(has)[0], cols[has]] = -1                            # below every rank: never among the top <= n - 1
    want = np.argsort(-r, axis=1, kind="stable")[:, :top]
    bad = np.argwhere(idx != want)
    assert len(bad) == 0, ("topk_rows self", keys.shape, top, ld, offset, col0, bad[0].tolist(), idx[bad[0][0]][:12], want[bad[0][0]][:12])
    assert np.array_equal(key, np.take_along_axis(keys, want, axis=1))
    assert np.array_equal(own[has], keys[np.nonzero(has)[0], cols[has]]) and not own[~has].any()      # self_key: the own element; untouched elsewhere


@pytest.mark.parametrize("n", [2, 3, 7, 64, 1024, 1025, 2048, 5000])
def test_topk_rows_self_layouts(da, n):
    rng = np.random.RandomState(n)
    ld8 = -(-n // 8) * 8
    # own columns from 0; ending at n - 1 (an unaligned tail unless n is a multiple of 8); inside a 16-byte unit; row 0 at -1; the last row at n
    col0s = sorted({0, n - ROWS, 3, -1, n - ROWS + 1})
    for col0 in col0s:
        keys = self_block(rng, n, col0, 40, 60000)
        for top in sorted({1, min(10, n - 1), min(1024, n - 1)}):
            for ld, offset in ((ld8, 0), (ld8 + 8, 8), (n + 1 - (n % 2), 0), (ld8, 3), (n, 1)):   # aligned, aligned, odd ld, unaligned base, both
                run_self(keys, top, ld, offset, col0, rank_bits=16)
    run_self(self_block(rng, n, 0, 40, 63), min(10, n - 1), ld8, 0, 0, rank_bits=6)               # one digit only


def test_topk_rows_self_with_a_rank_table_that_ties_distinct_keys(da):
    rng = np.random.RandomState(3)
    rank = (np.arange(65536) // 3).astype(np.uint16)                # three keys per rank
    for n, bits_ in ((500, 15), (1025, 15), (3000, 0)):
        for col0 in (0, n - ROWS, 250):
            keys = self_block(rng, n, col0, 2000, 60000)
            assert len(np.unique(rank[keys[4]])) < len(np.unique(keys[4]))
            for top in (1, 10, min(n - 1, 1024)):
                run_self(keys, top, -(-n // 8) * 8, 0, col0, rank=rank, rank_bits=bits_)
                run_self(keys, top, n + 1, 5, col0, rank=rank, rank_bits=bits_)


def test_topk_rows_self_refuses_top_equal_n_and_the_plain_form_is_unchanged(da):
    from dynaalign_amd import device
    keys = torch.from_numpy(np.arange(40, dtype=np.int16).reshape(4, 10).copy()).cuda()
    with pytest.raises(da.DynaAlignError) as e:
        device.topk_rows(keys, 10, self_col0=0)
    assert e.value.code == 11 and "n - 1" in str(e.value)
    idx, key = device.topk_rows(keys, 10)                           # top = n through the plain form
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(9, -1, -1, dtype=np.int32), (4, 1)))
    idx, key = device.topk_rows(keys, 9, self_col0=100)             # no own column in range: the plain selection
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(9, 0, -1, dtype=np.int32), (4, 1)))


# ---- MinHash -----------------------------------------------------------------------------------------------------------------------------------

def host_mh(seqs, k, n_hash, seeds, top, with_val=True):
    from dynaalign_amd import _capi
    res, off = O.pack(seqs)
    idx, val = np.full((len(seqs), top), -7, np.int32), np.full((len(seqs), top), -7.0)
    _capi.check(_capi.load().da_similarity_mh_knn(res.ctypes.data, off.ctypes.data, len(seqs), k, n_hash,
                                                  np.ascontiguousarray(seeds, np.uint32).ctypes.data, top, idx.ctypes.data,
                                                  val.ctypes.data if with_val else None))
    return idx, (val if with_val else None)


def device_mh(seqs, k, n_hash, seeds, top):
    from dynaalign_amd import device
    idx, val = device.similarity_mh_knn(device.DeviceSequences(*O.pack(seqs)), k, n_hash, seeds, top)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


MH_CASES = [(1, 1, 4, 50), (2, 3, 1, 33), (127, 129, 4, 500), (300, 1001, 4, 50)]


@pytest.mark.parametrize("m,n,k,n_hash", MH_CASES, ids=["%d+%d" % c[:2] for c in MH_CASES])
def test_minhash_every_entry_point_against_the_oracle(da, m, n, k, n_hash):
    from dynaalign_amd import session
    rng = np.random.RandomState(2000 + m)
    x, y = two_sets(rng, m, n, ALPHABET, high_bytes=True)
    seqs = x + y
    total = len(seqs)
    seeds = O.seeds(SEED, n_hash)
    rc, S = O.similarity_mh(seqs, k, n_hash, seeds)
    assert rc == 0 and np.array_equal(S, S.T)
    s = session.MinHashSession(seqs, k, n_hash, seed=SEED, reserve=False)
    sub = np.arange(total - 1, -1, -3)
    for top in sorted({min(t, total - 1, 1024) for t in (1, 2, 10, total - 1)}):
        assert_lists(da.similarityMH_knn(seqs, k, n_hash, top, seed=SEED), S, top, ("mirror", total, top))
        assert_lists(host_mh(seqs, k, n_hash, seeds, top), S, top, ("host", total, top))
        assert_lists(device_mh(seqs, k, n_hash, seeds, top), S, top, ("one call", total, top))
        assert_lists(s.knn(top), S, top, ("session", total, top))
        if len(sub) >= 2:
            t = min(top, len(sub) - 1)
            assert_lists(s.knn(top, sub), S[np.ix_(sub, sub)], t, ("session, subset", total, top))
    assert_lists(host_mh(seqs, k, n_hash, seeds, 1, with_val=False), S, 1, ("host, no values", total))
    if total - 1 <= 1024:                                               # the mirror clamps top to n - 1
        assert_lists(da.similarityMH_knn(seqs, k, n_hash, total + 7, seed=SEED), S, total - 1, ("mirror, clamped", total))


def test_minhash_identical_strings_list_each_other_in_position_order(da):
    """three byte-identical strings at a < b < c: row c lists [a, b] first at 1.0 -- the cross call on (x, x) with its first column dropped
    lists [b, c], because c's own column is the LAST of its ties there"""
    rng = np.random.RandomState(11)
    seqs = ["".join(ALPHABET[i] for i in rng.randint(0, 20, 12)) for _ in range(9)]
    a, b, c = 2, 5, 7
    seqs[b] = seqs[c] = seqs[a]
    seeds = O.seeds(SEED, 50)
    rc, S = O.similarity_mh(seqs, 4, 50, seeds)
    assert rc == 0
    for got in (da.similarityMH_knn(seqs, 4, 50, 3, seed=SEED), host_mh(seqs, 4, 50, seeds, 3), device_mh(seqs, 4, 50, seeds, 3)):
        assert_lists(got, S, 3, "identical strings")
        idx, val = got
        assert idx[c, :2].tolist() == [a, b] and idx[a, :2].tolist() == [b, c] and idx[b, :2].tolist() == [a, c]
        assert val[c, 0] == 1.0 and val[c, 1] == 1.0 and val[c, 2] < 1.0
    cross_idx, _ = da.similarityMH_cross_topk(seqs, seqs, 4, 50, 3, seed=SEED)
    assert cross_idx[c].tolist() == [a, b, c] and cross_idx[c, 1:].tolist() == [b, c]      # what cross-and-strip would list for row c


def test_minhash_knn_edges_mirror(da):
    rng = np.random.RandomState(12)
    x, y = two_sets(rng, 60, 70, ALPHABET)
    seqs = x + y
    rc, S = O.similarity_mh(seqs, 4, 50, O.seeds(SEED, 50))
    for mode in ("union", "mutual"):
        thr, i, j, w = da.similarityMH_knn_edges(seqs, 4, 50, 5, mode, seed=SEED)
        wi, wj, ww = da.knn_graph(*da.knn_dense(S, 5), 1.0, mode)
        assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(bits(w), bits(ww))
        off = ww[wi != wj]
        assert thr == off.min() and np.array_equal(bits(w[i != j]), bits(S[i[i != j], j[i != j]])) and (w[i == j] == 1.0).all()


# ---- NW ------------------------------------------------------------------------------------------------------------------------------------------

def host_nw(seqs, matrix, go, ge, top, with_diag=True):
    from dynaalign_amd import _capi
    res, off = O.pack(seqs)
    idx, val, diag = np.full((len(seqs), top), -7, np.int32), np.full((len(seqs), top), -7.0), np.full(len(seqs), -7.0)
    _capi.check(_capi.load().da_similarity_nw_knn(res.ctypes.data, off.ctypes.data, len(seqs), matrix.encode(), go, ge, top, idx.ctypes.data,
                                                  val.ctypes.data, diag.ctypes.data if with_diag else None))
    return idx, val, diag


@pytest.fixture(scope="module")
def nw_input():
    x, y = nw_sets(np.random.RandomState(901), 100, 160)
    seqs = x + y
    assert len(seqs) == 260 and min(map(len, seqs)) == 1 and max(map(len, seqs)) == 126
    return seqs


@pytest.fixture(scope="module")
def nw_oracle(nw_input):
    out = {}
    for matrix, go, ge in (("BLOSUM62", 10, 4), ("BLOSUM50", 11, 1)):
        rc, nm, ln, _, _ = O.nw_rows(nw_input, 0, len(nw_input), matrix, go, ge)
        assert rc == 0
        out[matrix] = (nm.astype(np.float64) / ln.astype(np.float64), (nm << 8) | ln)
    return out


def test_nw_oracle_input_exercises_ties_and_misplaced_self(da, nw_input, nw_oracle):
    S, code = nw_oracle["BLOSUM62"]
    n = len(nw_input)
    assert np.array_equal(bits(S), bits(S.T))
    rc, full, _ = O.similarity_nw(nw_input, "BLOSUM62", 10, 4)
    assert rc == 0 and np.array_equal(bits(full), bits(S))                                   # S IS the matrix similarityNW returns
    first = np.argsort(-S, axis=1, kind="stable")[:, 0]
    assert int((first != np.arange(n)).sum()) >= 50                                          # self is not the first of its ties (95)
    idx, val = da.knn_dense(S, 10)
    sel = np.take_along_axis(code, idx.astype(np.int64), axis=1)
    tied = (val[:, 1:] == val[:, :-1]) & (sel[:, 1:] != sel[:, :-1]) & (val[:, 1:] > 0)
    assert int(tied.sum()) >= 20, int(tied.sum())                                            # equal values, different codes (58)


@pytest.mark.parametrize("matrix,go,ge", [("BLOSUM62", 10, 4), ("BLOSUM50", 11, 1)])
def test_nw_against_the_oracle(da, nw_input, nw_oracle, matrix, go, ge):
    S, _ = nw_oracle[matrix]
    for top in (1, 10, 259):
        assert_lists(da.similarityNW_knn(nw_input, matrix, go, ge, top), S, top, ("NW mirror", matrix, top))
        idx, val, diag = host_nw(nw_input, matrix, go, ge, top)
        assert_lists((idx, val), S, top, ("NW host", matrix, top))
        assert np.array_equal(bits(diag), bits(np.diag(S).copy()))
    idx, val, _ = host_nw(nw_input, matrix, go, ge, 10, with_diag=False)
    assert_lists((idx, val), S, 10, ("NW host, no diagonal", matrix))
    assert_lists(da.similarityNW_knn(nw_input, matrix, go, ge, 300), S, 259, ("NW mirror, clamped", matrix))
    thr, i, j, w = da.similarityNW_knn_edges(nw_input, matrix, go, ge, 10, "union")
    wi, wj, ww = da.knn_graph(*da.knn_dense(S, 10), np.diag(S).copy(), "union")
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(bits(w), bits(ww)) and thr == ww[wi != wj].min()


# ---- row blocks ----------------------------------------------------------------------------------------------------------------------------------

def test_row_blocks_give_identical_results(da, nw_input, nw_oracle):
    k, n_hash, top = 4, 50, 10
    x, y = two_sets(np.random.RandomState(77), 100, 200, ALPHABET, high_bytes=True)
    seqs = x + y
    seeds = O.seeds(SEED, n_hash)
    rc, S = O.similarity_mh(seqs, k, n_hash, seeds)
    whole = (host_mh(seqs, k, n_hash, seeds, top), device_mh(seqs, k, n_hash, seeds, top))
    nw_whole = host_nw(nw_input, "BLOSUM62", 10, 4, top)
    with switches(DYNAALIGN_BLOCK_BYTES=1024):                     # 128-row blocks: self_col0 is 0, 128 and 256
        blocked = (host_mh(seqs, k, n_hash, seeds, top), device_mh(seqs, k, n_hash, seeds, top))
        nw_blocked = host_nw(nw_input, "BLOSUM62", 10, 4, top)
    for w, b in zip(whole, blocked):
        assert_lists(b, S, top, "blocked")
        assert np.array_equal(w[0], b[0]) and np.array_equal(bits(w[1]), bits(b[1]))
    assert_lists(nw_blocked[:2], nw_oracle["BLOSUM62"][0], top, "NW, blocked")
    assert all(np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b) for a, b in zip(nw_whole, nw_blocked))
    from dynaalign_amd import session
    s = session.MinHashSession(seqs, k, n_hash, seed=SEED, reserve=False)
    assert_lists(s.knn(top, block_bytes=1024), S, top, "session, blocked")


# ---- lists -> graph --------------------------------------------------------------------------------------------------------------------------------

def run_knn_edges(da, idx, val, key, mode, loops, is_nw, values, self_key=None, self_code=0):
    from dynaalign_amd import device
    idx_t = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    key_t = torch.from_numpy(np.ascontiguousarray(key, np.uint16).view(np.int16)).cuda()
    sk_t = None if self_key is None else torch.from_numpy(np.ascontiguousarray(self_key, np.uint16).view(np.int16)).cuda()
    ei, ej, ev, m = device.knn_edges(idx_t, key_t, mode, is_nw=is_nw, self_key=sk_t, self_code=self_code, loops=loops)
    torch.cuda.synchronize()
    ei, ej, ev = ei.cpu().numpy(), ej.cpu().numpy(), ev.cpu().numpy().view(np.uint16)
    assert len(ei) == m
    order = np.lexsort((ej, ei))
    diag = None if not loops else (values[self_key] if self_key is not None else values[self_code])
    wi, wj, ww = da.knn_graph(idx, val, diag, mode)
    assert np.array_equal(ei[order], wi) and np.array_equal(ej[order], wj), (mode, loops, is_nw, m, len(wi))
    assert np.array_equal(bits(values[ev[order]]), bits(ww))
    return ei, ej, ev


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_edges_equal_knn_graph(da, mode, nw_input, nw_oracle):
    n_hash = 50
    values = np.arange(n_hash + 1, dtype=np.float64) / n_hash
    for m, n, top in ((3, 4, 2), (60, 70, 5), (90, 110, 70), (90, 110, 199)):      # top >= 65: the membership scan loops
        x, y = two_sets(np.random.RandomState(300 + top), m, n, ALPHABET)
        seqs = x + y
        sig = O.signatures(seqs, 4, n_hash, O.seeds(SEED, n_hash))
        cnt = O.mh_counts(sig)
        S = cnt.astype(np.float64) / np.float64(n_hash)
        idx, val = da.knn_dense(S, top)
        key = np.take_along_axis(cnt, idx.astype(np.int64), axis=1)
        assert (val == 0).any() or top < 10                                       # zero-valued entries are in the lists, and dropped
        for loops in (True, False):
            run_knn_edges(da, idx, val, key, mode, loops, False, values, self_code=n_hash)
    S, code = nw_oracle["BLOSUM62"]
    nw_values = np.array([(c >> 8) / (c & 255) if c & 255 else 0.0 for c in range(65536)])
    for top in (3, 10, 80):
        idx, val = da.knn_dense(S, top)
        key = np.take_along_axis(code, idx.astype(np.int64), axis=1).astype(np.uint16)
        assert np.array_equal(bits(nw_values[key]), bits(val))
        for loops in (True, False):
            run_knn_edges(da, idx, val, key, mode, loops, True, nw_values, self_key=np.diag(code).astype(np.uint16))


def test_knn_edges_do_not_rely_on_symmetric_lists(da):
    # 0 is everybody's neighbour but lists only 1; row 3's entry has a zero key
    idx = np.array([[1], [0], [0], [0], [3]], np.int32)
    key = np.array([[45], [45], [25], [0], [10]], np.uint16)
    values = np.arange(51, dtype=np.float64) / 50
    ei, ej, ev = run_knn_edges(da, idx, values[key], key, "union", False, False, values)
    assert sorted(zip(ei.tolist(), ej.tolist(), ev.tolist())) == [(0, 1, 45), (0, 2, 25), (3, 4, 10)]
    ei, ej, ev = run_knn_edges(da, idx, values[key], key, "mutual", True, False, values, self_code=50)
    assert sorted(zip(ei.tolist(), ej.tolist(), ev.tolist())) == [(0, 0, 50), (0, 1, 45), (1, 1, 50), (2, 2, 50), (3, 3, 50), (4, 4, 50)]


def families(rng, n, fam, length=14):
    base = ["".join(ALPHABET[i] for i in rng.randint(0, 20, length)) for _ in range(fam)]
    out = []
    for t in range(n):
        s = list(base[t % fam])
        for _ in range(1 + t // fam % 3):
            s[rng.randint(0, length)] = ALPHABET[rng.randint(0, 20)]
        out.append("".join(s) + ALPHABET[t % 20] * (t // (20 * fam) % 3))
    return out


def test_session_knn_csr_clusters_like_the_edge_list(da):
    from dynaalign_amd import session
    seqs = families(np.random.RandomState(21), 400, 9)
    k, n_hash = 3, 64
    s = session.MinHashSession(seqs, k, n_hash, seed=SEED, reserve=False)
    for mode in ("union", "mutual"):
        thr, i, j, w = da.similarityMH_knn_edges(seqs, k, n_hash, 8, mode, seed=SEED)
        cthr, m, ptr, adj, codes, loops, values = s.knn_csr(None, 8, mode)
        assert m == len(i) and cthr == thr and ptr[-1] == 2 * int((i != j).sum())
        want = da.louvain(len(seqs), i, j, w, seed=5)
        got = da.louvain_csr(len(seqs), ptr, adj, codes, loops, values, seed=5)
        assert np.array_equal(got, want) and len(set(want.tolist())) > 1


def test_clusterbreak_with_knn_equals_the_edges_fn_form(da):
    from dynaalign_amd import session
    seqs = families(np.random.RandomState(22), 600, 5)
    k, n_hash = 3, 64
    s = session.MinHashSession(seqs, k, n_hash, seed=SEED, reserve=False)
    a = da.clusterbreak(seqs, size_max=50, session=s, knn=8, cluster_seed=2)
    b = da.clusterbreak(seqs, size_max=50, edges_fn=lambda sub: da.similarityMH_knn_edges(sub, k, n_hash, 8, seed=SEED), cluster_seed=2)
    assert np.array_equal(a["clustered_seq"], b["clustered_seq"]) and a["filtered_seq"] == b["filtered_seq"]
    assert a.calls == b.calls > 1 and [l["edges"] for l in a.levels] == [l["edges"] for l in b.levels]
    assert all(l["edges"] <= l["n"] * 9 for l in a.levels)                                    # at most n * top edges + the diagonal
    c = da.clusterbreak(seqs, size_max=50, session=s, knn=8, knn_mode="mutual", cluster_seed=2, cluster_fn=da.louvain)   # the edge-list way
    d = da.clusterbreak(seqs, size_max=50, edges_fn=lambda sub: da.similarityMH_knn_edges(sub, k, n_hash, 8, "mutual", seed=SEED), cluster_seed=2)
    assert np.array_equal(c["clustered_seq"], d["clustered_seq"]) and c["filtered_seq"] == d["filtered_seq"]
