"""Plain-Python yardstick for nw_align and clusterconsensus -- TEST INFRASTRUCTURE, written independently of the library.

`align(a, b, ...)` fills the reference's three full matrices and its traceback matrix (src/pairwiseSeqAlign.cpp:216-281) cell by cell and
walks the traceback from (m, n) (:284-308); it returns the decision string in forward order, the alignment length, the matches and
M[m][n].  `consensus(rows)` is the center-star rule of clusterconsensus on top of `align`.  Scores come from the stored BLOSUM tables
(tests/golden/blosum_tables.json), not from the library.  No numpy in the recurrences: every value is a Python int.
"""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_META = json.load(open(os.path.join(HERE, "golden", "blosum_tables.json")))
ORDER = _META["order"]                         # "ARNDCQEGHILKMFPSTWYVBZX*"
TABLES = {name: t["values"] for name, t in _META["tables"].items()}
MATRICES = sorted(TABLES)
NEG = -(2 ** 31) // 2                          # std::numeric_limits<int>::min() / 2
PENALTIES = [(10, 4), (0, 0), (1, 1), (3, 0), (200, 100)]
SYMBOLS = ORDER + "-"


def align(a, b, matrix="BLOSUM62", go=10, ge=4):
    """-> (ops, length, matches, score) of calc(a, b) with a as sequence1"""
    tab = TABLES[matrix]
    m, n = len(a), len(b)
    M = [[NEG] * (n + 1) for _ in range(m + 1)]
    Ix = [[NEG] * (n + 1) for _ in range(m + 1)]
    Iy = [[NEG] * (n + 1) for _ in range(m + 1)]
    tb = [["0"] * (n + 1) for _ in range(m + 1)]
    M[0][0] = 0
    for i in range(1, m + 1):
        Ix[i][0] = -go - (i - 1) * ge
        tb[i][0] = "U"
    for j in range(1, n + 1):
        Iy[0][j] = -go - (j - 1) * ge
        tb[0][j] = "L"
    for i in range(1, m + 1):
        ia = ORDER.index(a[i - 1])
        for j in range(1, n + 1):
            s = tab[ia * 24 + ORDER.index(b[j - 1])]
            Ix[i][j] = max(M[i - 1][j] - (go + ge), Ix[i - 1][j] - ge)
            Iy[i][j] = max(M[i][j - 1] - (go + ge), Iy[i][j - 1] - ge)
            d = max(M[i - 1][j - 1] + s, Ix[i - 1][j - 1] + s, Iy[i - 1][j - 1] + s)
            if d >= Ix[i][j] and d >= Iy[i][j]:
                M[i][j], tb[i][j] = d, "D"
            elif Ix[i][j] >= Iy[i][j]:
                M[i][j], tb[i][j] = Ix[i][j], "U"
            else:
                M[i][j], tb[i][j] = Iy[i][j], "L"
    ops, matches = [], 0
    i, j = m, n
    while i > 0 or j > 0:
        t = tb[i][j]
        ops.append(t)
        if t == "D":
            matches += a[i - 1] == b[j - 1]
            i, j = i - 1, j - 1
        elif t == "U":
            i -= 1
        else:
            j -= 1
    ops.reverse()
    return "".join(ops), len(ops), matches, M[m][n]


def gapped(a, b, ops):
    """the two gapped strings of a path"""
    ga = gb = ""
    i = j = 0
    for op in ops:
        if op == "D":
            ga, gb, i, j = ga + a[i], gb + b[j], i + 1, j + 1
        elif op == "U":
            ga, gb, i = ga + a[i], gb + "-", i + 1
        else:
            ga, gb, j = ga + "-", gb + b[j], j + 1
    assert i == len(a) and j == len(b)
    return ga, gb


def consensus_of(members, aligner=align):
    """center-star consensus of one cluster (members in input order, duplicates kept); aligner(a, b) -> (ops, length, matches, score)"""
    c = len(members)
    if c == 1:
        return members[0]
    sums = []
    for i in range(c):
        terms = []
        for j in range(c):
            if j != i:
                _, ln, mt, _ = aligner(members[i], members[j])
                terms.append(mt / ln if ln else 0.0)
        sums.append(math.fsum(terms))
    ci = max(range(c), key=lambda i: (sums[i], -i))          # largest sum, lowest index among equals
    cen = members[ci]
    columns = [[ch] for ch in cen]
    for j in range(c):
        if j == ci:
            continue
        ops = aligner(cen, members[j])[0]
        p = q = 0
        for op in ops:
            if op == "D":
                columns[p].append(members[j][q])
                p, q = p + 1, q + 1
            elif op == "U":
                columns[p].append("-")
                p += 1
            else:
                q += 1
    out = ""
    for p, col in enumerate(columns):
        top = max(col.count(s) for s in set(col))
        tied = {s for s in set(col) if col.count(s) == top}
        win = cen[p] if cen[p] in tied else next(s for s in SYMBOLS if s in tied)
        if win != "-":
            out += win
    return out


def consensus(rows, aligner=align):
    """rows of (sequence, cluster_id) -> [(cluster_id, consensus)] in first-appearance order of the ids"""
    ids, groups = [], {}
    for seq, cid in rows:
        if cid not in groups:
            groups[cid] = []
            ids.append(cid)
        groups[cid].append(seq)
    return [(cid, consensus_of(groups[cid], aligner)) for cid in ids]


# ---- inputs the tests share -------------------------------------------------------------------------------------------------------
def random_seq(rng, length, alphabet=ORDER[:20]):
    return "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), length))


def mutate(rng, s, alphabet=ORDER[:20], rate=0.15, max_len=127):
    """a copy of s with substitutions, deletions and insertions (at most max_len residues)"""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(alphabet[int(rng.integers(0, len(alphabet)))])
            continue
        out.append(ch)
        if u > 1 - rate / 3:
            out.append(alphabet[int(rng.integers(0, len(alphabet)))])
    return "".join(out)[:max_len]
