"""The yardstick of nw_align / clusterconsensus, pinned without a GPU: the plain-Python full-matrix model (tests/nw_align_model.py)
against the CPU oracle's (matches, length, score), against the known answers, and its consensus rule against hand-checked cases."""
import numpy as np
import pytest

import nw_align_model as model
import oracle_lib as O


def test_the_tables_are_the_reference_order_and_all_six():
    assert model.ORDER == "ARNDCQEGHILKMFPSTWYVBZX*"
    assert model.MATRICES == sorted(["BLOSUM45", "BLOSUM50", "BLOSUM62", "BLOSUM80", "BLOSUM90", "BLOSUM100"])
    assert all(len(model.TABLES[k]) == 576 for k in model.MATRICES)
    assert model.NEG == -1073741824


def oracle_cases():
    """360 pairs: every matrix x every penalty pair x 12 pairs -- random and mutated content, lengths 0 .. 127 with the ends forced"""
    rng = np.random.default_rng(20261017)
    forced = [(0, 0), (0, 9), (9, 0), (1, 1), (127, 127), (127, 1), (1, 127), (127, 64)]
    out, k = [], 0
    for matrix in model.MATRICES:
        for go, ge in model.PENALTIES:
            for t in range(12):
                if t == 0:
                    la, lb = forced[k % len(forced)]
                    k += 1
                else:
                    la, lb = (int(v) for v in rng.integers(0, 128, 2))
                alphabet = model.ORDER if t % 3 else model.ORDER[:2]          # all 24 symbols, or two letters (ties)
                a = model.random_seq(rng, la, alphabet)
                b = model.mutate(rng, a, alphabet) if t % 2 else model.random_seq(rng, lb, alphabet)
                out.append((a, b, matrix, go, ge))
    return out


def test_model_agrees_with_the_oracle_on_matches_length_score(built):
    cases = oracle_cases()
    assert len(cases) == 360
    lengths = {len(c[0]) for c in cases} | {len(c[1]) for c in cases}
    assert 0 in lengths and 127 in lengths
    for a, b, matrix, go, ge in cases:
        ops, ln, mt, sc = model.align(a, b, matrix, go, ge)
        rc, omt, oln, osc, _ = O.nw_pair(a, b, matrix, go, ge)
        assert rc == 0
        assert (mt, ln, sc) == (omt, oln, osc), (a, b, matrix, go, ge)
        # the path is consistent with its own summary
        assert len(ops) == ln and ops.count("D") + ops.count("U") == len(a) and ops.count("D") + ops.count("L") == len(b)
        ga, gb = model.gapped(a, b, ops)
        assert sum(x == y for x, y in zip(ga, gb)) == mt


KNOWN = [
    ("YDYIHIYADKQDRIGWLGNT", "MYCEMNVEIQYMATKNMWNT", "BLOSUM62", 10, 4, 3, 21, "LDDDDDDDDDDDDDDDUDDDD", -17),
    ("MYCEMNVEIQYMATKNMWNT", "YDYIHIYADKQDRIGWLGNT", "BLOSUM62", 10, 4, 4, 21, "LDDDDDDDDDDDDDDDUDDDD", -17),
    ("PPPSYETVMAAA", "TPPPSYETVMAA", "BLOSUM62", 10, 4, 11, 13, "LDDDDDDDDDUDD", 35),
]


@pytest.mark.parametrize("a,b,matrix,go,ge,mt,ln,ops,sc", KNOWN)
def test_known_answers(a, b, matrix, go, ge, mt, ln, ops, sc):
    assert model.align(a, b, matrix, go, ge) == (ops, ln, mt, sc)


def test_known_answers_are_the_stored_ones(kats):
    k = kats["nw_asymmetric"]
    assert (k["a"], k["b"]) == KNOWN[0][:2] and k["ab"] == [KNOWN[0][5], KNOWN[0][6]] and k["ba"] == [KNOWN[1][5], KNOWN[1][6]]
    s = kats["nw_4x4"]["sequences"]
    assert (s[1], s[2]) == KNOWN[2][:2] and kats["nw_4x4"]["exact_fractions"]["1,2"] == [KNOWN[2][5], KNOWN[2][6]]


def test_known_tie_path():
    assert model.align("ACACCA", "CAACAC", "BLOSUM45", 0, 0)[0] == "UDLDDLDU"


def test_empty_sides():
    assert model.align("", "") == ("", 0, 0, 0)
    assert model.align("", "ACD") == ("LLL", 3, 0, model.NEG)
    assert model.align("AC", "") == ("UU", 2, 0, model.NEG)


def test_gapped_strings():
    assert model.gapped("PPPSYETVMAAA", "TPPPSYETVMAA", "LDDDDDDDDDUDD") == ("-PPPSYETVMAAA", "TPPPSYETVM-AA")


# ---- the consensus rule, hand-checked -------------------------------------------------------------------------------------------
CORE = "MKTAYIAKQRQISFVK"


def test_consensus_single_member_is_itself():
    assert model.consensus([("ACDEFGHIK", "7")]) == [("7", "ACDEFGHIK")]


def test_consensus_tie_goes_to_the_center():
    # two members, both sums 3/4: the center is member 0; position 3 has E : F = 1 : 1 and the center's E wins
    assert model.align("ACDE", "ACDF")[:3] == ("DDDD", 4, 3) and model.align("ACDF", "ACDE")[:3] == ("DDDD", 4, 3)
    assert model.consensus_of(["ACDE", "ACDF"]) == "ACDE"
    assert model.consensus_of(["ACDF", "ACDE"]) == "ACDF"


def test_consensus_tie_without_the_center_goes_by_symbol_order():
    # member 0 is 6/8 from every other one (sum 3.0); the others are 6/8, 6/8, 5/8, 5/8 from the rest (2.75): member 0 is the center.
    # position 4 holds C (center) : A : S = 1 : 2 : 2 -- the center is not among the tied, A comes before S in ARNDCQEGHILKMFPSTWYVBZX*-
    mem = ["KKKKCKKK", "RKKKAKKK", "KRKKAKKK", "KKRKSKKK", "KKKRSKKK"]
    for o in mem[1:]:
        assert model.align(mem[0], o)[:3] == ("D" * 8, 8, 6)
    assert model.align(mem[1], mem[3])[:3] == ("D" * 8, 8, 5)
    assert model.consensus_of(mem) == "KKKKAKKK"


def test_consensus_position_won_by_a_gap_is_dropped():
    # member 0 = W + core; members 1 and 2 are the core with one substitution each, at different places.  Sums: 15/17 + 15/17 for member
    # 0 against 15/17 + 14/16 for the others: member 0 is the center.  Its W stands opposite a gap in both alignments: W : - = 1 : 2
    b, c = CORE[:3] + "W" + CORE[4:], CORE[:9] + "W" + CORE[10:]
    mem = ["W" + CORE, b, c]
    assert model.align(mem[0], b)[:3] == ("U" + "D" * 16, 17, 15)
    assert model.align(mem[0], c)[:3] == ("U" + "D" * 16, 17, 15)
    assert model.align(b, c)[:3] == ("D" * 16, 16, 14)
    assert model.consensus_of(mem) == CORE


def test_consensus_inserted_residues_are_ignored():
    # the core is the center (15/16 + 16/17 against 15/16 + 15/17 and 16/17 + 15/17); the third member's extra W is an L step
    mem = [CORE[:3] + "W" + CORE[4:], CORE, "W" + CORE]
    assert model.align(CORE, mem[2])[0] == "L" + "D" * 16
    assert model.consensus_of(mem) == CORE


def test_consensus_duplicates_are_kept_and_ids_keep_their_first_appearance_order():
    rows = [("ACDEG", "b"), ("ACDEF", "a"), ("ACDEF", "b"), ("ACDEF", "b"), ("WWWW", 3)]
    # cluster b: ACDEG, ACDEF, ACDEF -- sums 1.6, 1.8, 1.8: the center is the first ACDEF; F : G = 2 : 1
    assert model.consensus(rows) == [("b", "ACDEF"), ("a", "ACDEF"), (3, "WWWW")]
