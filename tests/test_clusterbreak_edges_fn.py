"""CPU tests of clusterbreak's ``edges_fn`` hook: a level's thresholded graph handed over as an edge list gives the run the dense ``sim_fn``
path gives -- same labels, same filtered sequences, same number of calls, and per level the same threshold (bit for bit, NaN included) and
edge count.  The similarity is a deterministic numpy function of the strings; no device is needed (the clustering step is host code)."""
import io

import numpy as np
import pytest


@pytest.fixture(scope="module")
def cb(built):
    import importlib
    return importlib.import_module("dynaalign_amd.clusterbreak")     # the package attribute of that name is the function


def planted():
    """84 strings of 12 letters in 3 families x 4 subfamilies x 7 members: positions 0-3 the family, 4-6 the subfamily, the rest random"""
    rng = np.random.RandomState(5)
    return [a * 4 + b * 3 + "".join("KLMNPQ"[t] for t in rng.randint(0, 6, 5)) for a in "ACD" for b in "EFGH" for _ in range(7)]


def identity(seqs):
    """fraction of equal positions: symmetric, 1.0 on the diagonal, few distinct values"""
    a = np.array([list(s) for s in seqs])
    return (a[:, None, :] == a[None, :, :]).sum(axis=2) / 12.0


def levels_of(res):
    return [(lv["itr"], lv["n"], np.float64(lv["threshold"]).view(np.uint64), lv["edges"], lv["clusters"], lv["oversize"]) for lv in res.levels]


# the reference's defaults; a run in which EVERY cluster is broken again (size_max = 0), down to levels of a single sequence, until max_itr stops it
@pytest.mark.parametrize("kw", [dict(size_max=10, size_min=3), dict(size_max=4, size_min=1), dict(size_max=0, size_min=-1, max_itr=60)],
                         ids=["defaults", "small_clusters", "down_to_one_sequence"])
def test_edges_fn_gives_the_run_of_the_dense_path(cb, kw):
    pep = planted()
    p = 0.8
    seen = []

    def edges_fn(s):
        seen.append(len(s))
        return cb.threshold_edges_dense(identity(s), p)
    dense = cb.clusterbreak(pep, p, sim_fn=identity, log=io.StringIO(), **kw)
    edges = cb.clusterbreak(pep, p, edges_fn=edges_fn, log=io.StringIO(), **kw)
    assert np.array_equal(dense["clustered_seq"], edges["clustered_seq"]) and dense["filtered_seq"] == edges["filtered_seq"]
    assert (dense.calls, dense.convergence) == (edges.calls, edges.convergence)
    assert levels_of(dense) == levels_of(edges)
    sizes = [lv["n"] for lv in edges.levels]
    assert len(sizes) >= 3 and sizes[0] == len(pep) and sizes[1] < sizes[0]
    assert seen == [m for m in sizes if m >= 2]                      # called on every level of two or more sequences, on no other
    if kw["size_max"] == 0:
        # at least two levels below the first, then a level with one sequence: NaN threshold, the diagonal only
        assert sizes[:4] == sorted(sizes[:4], reverse=True) and len(set(sizes[:4])) >= 3 and 1 in sizes
        one = [lv for lv in edges.levels if lv["n"] == 1]
        assert all(np.isnan(lv["threshold"]) and lv["edges"] == 1 and lv["clusters"] == 1 for lv in one)
        assert edges.convergence == 0
    else:
        assert edges.convergence == 1 and min(sizes) >= 2


def test_edges_fn_replaces_sim_fn_and_excludes_a_session(cb):
    pep = planted()

    def never(s):
        raise AssertionError("sim_fn is not used when edges_fn is given")
    res = cb.clusterbreak(pep, 0.8, sim_fn=never, edges_fn=lambda s: cb.threshold_edges_dense(identity(s), 0.8))
    assert res.calls == cb.clusterbreak(pep, 0.8, sim_fn=identity).calls

    class FakeSession:
        n = len(pep)
    with pytest.raises(ValueError, match="edges_fn"):
        cb.clusterbreak(pep, 0.8, session=FakeSession(), edges_fn=lambda s: cb.threshold_edges_dense(identity(s), 0.8))
    # lists in place of arrays are taken as they are
    as_lists = cb.clusterbreak(pep, 0.8, edges_fn=lambda s: tuple(np.asarray(a).tolist() for a in cb.threshold_edges_dense(identity(s), 0.8)))
    assert np.array_equal(as_lists["clustered_seq"], res["clustered_seq"])
