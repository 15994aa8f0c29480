"""--distances restated in plain numpy, from the rule's text (include/bronko_hip.h, bk_cohort_set) and not from the kernels: letter
by letter, no bit planes, no popcounts.

  base       a byte is a base iff it is exactly A, C, G or T; every other byte is not comparable
  compared   compared[i][j] = positions at which both letters are bases; diff[i][j] = those of them at which the two differ
  clusters   i != j are linked iff diff[i][j] <= T and float(compared[i][j]) >= B * float(positions); clusters are the connected
             components, numbered from 1 in the order of their first sample
  files      <genome>.distances.tsv / .compared.tsv: "sample" and the names, then a line per sample: its name and its row;
             <genome>.clusters.tsv: ##cluster_threshold=T, ##cluster_min_breadth=B, "sample cluster size", a line per sample
"""
import numpy as np

ALPHABET = b"ACGTN-RYKMacgt" + bytes([200])   # what the tests draw letters from: bases, N, '-', ambiguity codes, lower case, a byte >= 128


def distances(letters):
    """(diff, compared), two (n, n) uint32 arrays, of an (n, positions) uint8 array."""
    a = np.asarray(letters, np.uint8)
    n = a.shape[0]
    base = (a == ord("A")) | (a == ord("C")) | (a == ord("G")) | (a == ord("T"))
    diff = np.zeros((n, n), np.uint32)
    compared = np.zeros((n, n), np.uint32)
    for i in range(n):
        both = base[i][None, :] & base
        compared[i] = both.sum(axis=1)
        diff[i] = (both & (a != a[i][None, :])).sum(axis=1)
    return diff, compared


def clusters(diff, compared, positions, threshold, min_breadth):
    """(cluster number per sample, cluster size per sample): a breadth-first walk of the link graph from every sample not yet reached."""
    n = len(diff)
    number = [0] * n
    members = {}
    for first in range(n):
        if number[first]:
            continue
        c = len(members) + 1
        number[first] = c
        members[c] = [first]
        todo = [first]
        while todo:
            i = todo.pop()
            for j in range(n):
                if j != i and not number[j] and int(diff[i][j]) <= threshold and float(compared[i][j]) >= min_breadth * float(positions):
                    number[j] = c
                    members[c].append(j)
                    todo.append(j)
    return number, [len(members[c]) for c in number]


def matrix_text(names, m):
    out = ["\t".join(["sample"] + list(names))]
    for name, row in zip(names, m):
        out.append("\t".join([name] + [str(int(v)) for v in row]))
    return ("\n".join(out) + "\n").encode()


def clusters_text(names, number, size, threshold, min_breadth):
    out = ["##cluster_threshold=%d" % threshold, "##cluster_min_breadth=%g" % min_breadth, "sample\tcluster\tsize"]
    for name, c, s in zip(names, number, size):
        out.append("%s\t%d\t%d" % (name, c, s))
    return ("\n".join(out) + "\n").encode()


def cohort(n, positions, seed):
    """The tests' cohort of n samples: related samples (one base sequence of ACGT with a handful of substitutions and a few
    letters from ALPHABET each), and -- as n allows -- an all-N sample, two identical samples and two samples that differ everywhere."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = acgt[rng.integers(0, 4, positions)]
    a = np.tile(base, (n, 1))
    alpha = np.frombuffer(ALPHABET, np.uint8)
    for s in range(n):
        k = int(rng.integers(0, 6))
        at = rng.integers(0, positions, k)
        a[s, at] = acgt[rng.integers(0, 4, k)]
        k = int(rng.integers(0, max(2, positions // 8)))
        at = rng.integers(0, positions, k)
        a[s, at] = alpha[rng.integers(0, len(alpha), k)]
    if n >= 2:
        a[n - 1] = a[0]                                      # two identical samples
    if n >= 3:
        a[1] = ord("N")                                      # an all-N sample
    if n >= 5:                                               # two samples that differ everywhere: every base rotated by one
        a[2] = base
        a[3] = acgt[(np.searchsorted(acgt, base) + 1) % 4]
    return np.ascontiguousarray(a)
