"""The yardstick of nw_align_long, pinned without a GPU ABOVE 127 residues (tests/test_nw_align_model.py stops there): the plain-Python
full-matrix model (tests/nw_align_model.py) against the CPU oracle's (matches, length, score) on lengths 0 .. 1024.  The model costs a few
microseconds per cell, so most pairs have one long side and only a handful have two."""
import numpy as np

import nw_align_model as model
import oracle_lib as O

FORCED = [(1024, 1024), (1024, 1), (1, 1024), (566, 567), (0, 700), (700, 0)]
MATRICES = ["BLOSUM62", "BLOSUM45"]
PENALTIES = [(10, 4), (0, 0)]


def long_cases():
    """40 pairs: the forced shapes, 30 with one side drawn from 0 .. 1024 and the other from 0 .. 40, 4 with both sides in 128 .. 300"""
    rng = np.random.default_rng(20261018)
    shapes = list(FORCED)
    for t in range(30):
        long_side, short_side = int(rng.integers(0, 1025)), int(rng.integers(0, 41))
        shapes.append((long_side, short_side) if t % 2 else (short_side, long_side))
    for t in range(4):
        shapes.append(tuple(int(v) for v in rng.integers(128, 301, 2)))
    out = []
    for t, (la, lb) in enumerate(shapes):
        alphabet = model.ORDER[:2] if t % 5 == 4 else model.ORDER          # two letters: ties
        a = model.random_seq(rng, la, alphabet)
        if t % 2 and min(la, lb) > 100:                                     # a mutated copy of a, cut or extended to lb residues
            b = model.mutate(rng, a, alphabet, max_len=2000)
            b = (b + model.random_seq(rng, max(lb - len(b), 0), alphabet))[:lb]
        else:
            b = model.random_seq(rng, lb, alphabet)
        go, ge = PENALTIES[(t // 2) % 2]
        out.append((a, b, MATRICES[t % 2], go, ge))
    return out


def test_model_agrees_with_the_oracle_above_127_residues(built):
    cases = long_cases()
    assert len(cases) == 40
    shapes = [(len(c[0]), len(c[1])) for c in cases]
    assert shapes[:6] == FORCED
    assert {c[2] for c in cases} == set(MATRICES) and {c[3:] for c in cases} == set(PENALTIES)
    assert {(c[2],) + c[3:] for c in cases} == {(m,) + p for m in MATRICES for p in PENALTIES}
    assert sum(min(s) > 127 for s in shapes) <= 8                          # both long: few
    assert sum(max(s) > 127 for s in shapes) >= 30
    for a, b, matrix, go, ge in cases:
        ops, ln, mt, sc = model.align(a, b, matrix, go, ge)
        rc, omt, oln, osc, _ = O.nw_pair(a, b, matrix, go, ge)
        assert rc == 0
        assert (mt, ln, sc) == (omt, oln, osc), (len(a), len(b), matrix, go, ge)
        # the path is consistent with its own summary
        assert len(ops) == ln and ops.count("D") + ops.count("U") == len(a) and ops.count("D") + ops.count("L") == len(b)
        i = j = same = 0
        for op in ops:
            same += op == "D" and a[i] == b[j]
            i += op != "L"
            j += op != "U"
        assert same == mt
