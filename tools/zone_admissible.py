#!/usr/bin/env python3
"""What the duplicate plan's id order means for the pipelined row expansion, on the CPU (no GPU, no library): for every cut of the default
schedule (head 1 band, then 8 bands a launch, 1024 table rows a band) the work items of each of the eight row zones that a launch may take
(table row below the cut) with ids by first occurrence and with the zoned order (multi-copy strings first, single-copy ones dealt round-robin
over the zones), and the output rows they cover.
usage: zone_admissible.py [n] [gen]      (default: 100000 h3n2_like, the headline input)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from dynaalign_amd import synth

ZONES, COPIES, BAND = 8, 4, 1024


def orders(seqs):
    """(ids by first occurrence, zoned ids, M) of a list of byte strings"""
    n = len(seqs)
    _, rep, inv, cnt = np.unique(np.array(seqs, dtype=object), return_index=True, return_inverse=True, return_counts=True)
    first_row = rep[inv]                                                   # first occurrence of every row's string
    reps = np.sort(rep)                                                    # the representatives' rows, ascending
    copies = cnt[inv][reps]
    first = np.empty(n, np.int64)
    first[reps] = np.arange(len(reps))
    multi, single = reps[copies > 1], reps[copies == 1]
    M = len(multi)
    Z = -(-n // ZONES)
    z = single // Z
    q = np.arange(len(single)) - np.searchsorted(single, z * Z)            # rank among the singles of its zone
    zoned = np.empty(n, np.int64)
    zoned[multi] = np.arange(M)
    zoned[single[np.lexsort((z, q))]] = M + np.arange(len(single))         # the rank of (q, z) in lexicographic order
    return first[first_row], zoned[first_row], M


def admissible(uidx, U, cuts):
    n = len(uidx)
    Z = -(-n // ZONES)
    c = np.bincount((np.arange(n) // Z) * U + uidx, minlength=ZONES * U).reshape(ZONES, U)
    items = np.cumsum(-(-c // COPIES), axis=1)
    rows = np.cumsum(c, axis=1)
    return [(items[:, min(U, b * BAND) - 1], int(rows[:, min(U, b * BAND) - 1].sum())) for b in cuts]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    gen = sys.argv[2] if len(sys.argv) > 2 else "h3n2_like"
    res, off = getattr(synth, gen)(n, 20)
    raw = np.asarray(res, np.uint8).tobytes()
    seqs = [raw[off[i]:off[i + 1]] for i in range(n)]
    first, zoned, M = orders(seqs)
    U = int(first.max()) + 1
    KB = -(-U // BAND)
    cuts = [1]
    while cuts[-1] < KB:
        cuts.append(min(KB, cuts[-1] + 8))
    print("n = %d, U = %d (%d multi-copy), %d bands, items in all: %d" % (n, U, M, KB, admissible(first, U, [KB])[0][0].sum()))
    print("| cut (bands done) | first occurrence: items per zone min .. max (output rows) | zoned: min .. max (output rows) |\n|---|---|---|")
    for b, (fi, fr), (zi, zr) in zip(cuts, admissible(first, U, cuts), admissible(zoned, U, cuts)):
        print("| %d | %d .. %d (%d) | %d .. %d (%d) |" % (b, fi.min(), fi.max(), fr, zi.min(), zi.max(), zr))


if __name__ == "__main__":
    main()
