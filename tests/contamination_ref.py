"""--contamination restated in plain numpy, from the rule's text (include/bronko_hip.h, bk_sample_minor_alleles and
bk_cohort_set_minor) and not from the kernels: letter by letter and mask by mask, no bit planes, no popcounts.

  present mask  per position, tot[b] = forward + reverse depth of base b, depth = their sum; bit b (A = 1, C = 2, G = 4, T = 8) iff
                tot[b] >= R and float(tot[b]) >= F * float(depth); mixed = positions with two bits or more, present = the set bits
  cons_i(p)     the consensus letter if it is exactly one of ACGT, else none
  minor_i(p)    empty if cons_i(p) is none, else the mask's low four bits without the bit of cons_i(p)
  explained     explained[i][j] = positions at which cons_i and cons_j are both bases, differ, and the bit of cons_j is in minor_i
  minor_sites   minor_sites[i] = positions with minor_i not empty
  best          best[i] = the j != i with the largest explained[i][j] >= 1; ties: the smaller diff[i][j], then the earlier sample
  flagged       (i, j), i != j, iff explained[i][j] >= S and float(explained[i][j]) >= P * float(diff[i][j])
  files         <genome>.explained.tsv: the layout of .distances.tsv; <genome>.contamination.tsv and <genome>.mixture.tsv: four ## lines,
                a header, a line per flagged pair / per sample; ratios from the integers, four decimals, truncated
"""
import numpy as np

from tests import cohort_ref

BIT = {ord("A"): 1, ord("C"): 2, ord("G"): 4, ord("T"): 8}
TALLIES = ("positions", "mixed", "present")


def present_masks(fwd, rev, min_reads, min_freq):
    """(masks as a uint8 array, {tally: count}) of `positions` consecutive cells: fwd and rev hold four counts a cell."""
    fwd = np.asarray(fwd).reshape(-1, 4).tolist()
    rev = np.asarray(rev).reshape(-1, 4).tolist()
    masks = np.zeros(len(fwd), np.uint8)
    t = dict.fromkeys(TALLIES, 0)
    for p, (f, r) in enumerate(zip(fwd, rev)):
        tot = [int(f[b]) + int(r[b]) for b in range(4)]
        depth = sum(tot)
        mask = 0
        for b in range(4):
            if tot[b] >= min_reads and float(tot[b]) >= min_freq * float(depth):
                mask |= 1 << b
        masks[p] = mask
        bits = bin(mask).count("1")
        t["positions"] += 1
        t["mixed"] += bits >= 2
        t["present"] += bits
    return masks, t


def _bits(letters):
    """The bit of every letter that is a base, 0 elsewhere."""
    a = np.asarray(letters, np.uint8)
    out = np.zeros(a.shape, np.uint8)
    for ch, bit in BIT.items():
        out[a == ch] = bit
    return out


def minor(letters, masks):
    """minor_i(p) of every sample and position, as the mask's bits."""
    bit = _bits(letters)
    return np.where(bit != 0, (np.asarray(masks, np.uint8) & 15) & ~bit, 0).astype(np.uint8)


def explained(letters, masks):
    """(explained, minor_sites): an (n, n) and an (n,) uint32 array of two (n, positions) uint8 arrays."""
    a = np.asarray(letters, np.uint8)
    bit, mn = _bits(a), minor(a, masks)
    n = a.shape[0]
    ex = np.zeros((n, n), np.uint32)
    for i in range(n):
        both = (bit[i] != 0)[None, :] & (bit != 0)
        ex[i] = (both & (a != a[i][None, :]) & ((mn[i][None, :] & bit) != 0)).sum(axis=1)
    return ex, (mn != 0).sum(axis=1).astype(np.uint32)


def scan(diff, ex, min_sites, min_share):
    """(flagged [(i, j)] ordered by (i, j), best [j or None] per sample, the sources every sample is flagged for)."""
    n = len(diff)
    flagged, best, counts = [], [], [0] * n
    for i in range(n):
        cand = [(-int(ex[i][j]), int(diff[i][j]), j) for j in range(n) if j != i and int(ex[i][j]) >= 1]
        best.append(min(cand)[2] if cand else None)
        for j in range(n):
            if j != i and int(ex[i][j]) >= min_sites and float(ex[i][j]) >= min_share * float(diff[i][j]):
                flagged.append((i, j))
                counts[i] += 1
    return flagged, best, counts


def ratio4(x, y):
    x, y = int(x), int(y)
    return "%d.%04d" % (x // y, x % y * 10000 // y)


def _head(min_reads, min_freq, min_sites, min_share):
    return ["##minor_min_reads=%d" % min_reads, "##minor_min_freq=%g" % min_freq, "##contamination_min_sites=%d" % min_sites,
            "##contamination_min_share=%g" % min_share]


explained_text = cohort_ref.matrix_text


def contamination_text(names, diff, compared, ex, sites, min_reads, min_freq, min_sites, min_share):
    out = _head(min_reads, min_freq, min_sites, min_share) + ["recipient\tsource\tdiff\tcompared\texplained\tshare\tminor_sites\tminor_share"]
    for i, j in scan(diff, ex, min_sites, min_share)[0]:
        out.append("%s\t%s\t%d\t%d\t%d\t%s\t%d\t%s" % (names[i], names[j], diff[i][j], compared[i][j], ex[i][j], ratio4(ex[i][j], diff[i][j]), sites[i],
                                                     ratio4(ex[i][j], sites[i])))
    return ("\n".join(out) + "\n").encode()


def mixture_text(names, diff, ex, sites, min_reads, min_freq, min_sites, min_share):
    out = _head(min_reads, min_freq, min_sites, min_share) + ["sample\tminor_sites\tflagged\tbest_source\texplained\tdiff\tshare"]
    _, best, counts = scan(diff, ex, min_sites, min_share)
    for i, name in enumerate(names):
        j = best[i]
        tail = ".\t.\t.\t." if j is None else "%s\t%d\t%d\t%s" % (names[j], ex[i][j], diff[i][j], ratio4(ex[i][j], diff[i][j]))
        out.append("%s\t%d\t%d\t%s" % (name, sites[i], counts[i], tail))
    return ("\n".join(out) + "\n").encode()


def cohort(n, positions, seed):
    """(letters, masks): cohort_ref.cohort(n, positions, seed) and a mask per letter -- random bytes 0..255, so the upper four bits are
    exercised -- with, as n allows: sample 2's mask 15 everywhere (it differs from sample 3 everywhere: explained = diff = positions),
    the last sample's mask 0 everywhere, sample 0's minor alleles exactly its differences from sample n - 2, and the all-N sample 1."""
    a = cohort_ref.cohort(n, positions, seed)
    rng = np.random.default_rng(seed + 7)
    m = rng.integers(0, 256, a.shape).astype(np.uint8)
    if n >= 5:
        m[2] = 15 | (m[2] & 0xf0)
    if n >= 2:
        m[n - 1] = m[n - 1] & 0xf0
    if n >= 4:
        bit = _bits(a)
        s = n - 2
        differ = (bit[0] != 0) & (bit[s] != 0) & (a[0] != a[s])
        m[0] = (m[0] & 0xf0) | bit[0] | np.where(differ, bit[s], 0)
    return a, np.ascontiguousarray(m)
