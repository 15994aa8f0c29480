"""The contract of --adapter restated in Python (tests only): the cut position of a read, letter by letter and with numpy, the
truncated reads every result is defined by, the counters as the engine takes them on its records, and reads to try it all on."""
import math

import numpy as np

from tests import primer_ref

MAXB = primer_ref.MAXB   # bases of the longest record: a longer run of valid letters is cut into chunks and is not searched
PRESETS = {"truseq": b"AGATCGGAAGAGC", "nextera": b"CTGTCTCTTATACACATCT"}


def allowed(E, l):
    """floor(E * l), the product taken in double"""
    return int(math.floor(E * float(l)))


def cut_position(read, adapters, O, E, qual=None, min_qual=0, maxb=MAXB):
    """The letters the read keeps (s1 + p), or -1 if no adapter matches: letter by letter as the contract states it."""
    read = bytes(read)
    n = len(read)
    _, s1 = primer_ref.end_runs(read, qual, min_qual)
    R = read[s1:].upper()
    r = n - s1
    if r > maxb:
        return -1
    for p in range(0, r - O + 1):
        for A in adapters:
            A = bytes(A).upper()
            l = min(len(A), r - p)
            if primer_ref.hamming(R[p:p + l], A[:l]) <= allowed(E, l):
                return s1 + p
    return -1


def cut_positions_all(reads, adapters, O, E, quals=None, min_qual=0, maxb=MAXB):
    """cut_position for many reads (numpy over the positions of a read): arrays cut (-1: none) and s1"""
    ads = [np.frombuffer(bytes(A).upper(), np.uint8) for A in adapters]
    al = np.array([allowed(E, l) for l in range(65)], np.int64)
    cuts = np.full(len(reads), -1, np.int64)
    s1s = np.zeros(len(reads), np.int64)
    for i, read in enumerate(reads):
        read = bytes(read)
        _, s1 = primer_ref.end_runs(read, None if quals is None else quals[i], min_qual)
        s1s[i] = s1
        r = len(read) - s1
        if r < O or r > maxb:
            continue
        R = np.frombuffer(read[s1:].upper(), np.uint8)
        npos = r - O + 1
        best = -1
        for A in ads:
            LA = len(A)
            win = np.lib.stride_tricks.sliding_window_view(np.concatenate([R, np.zeros(LA, np.uint8)]), LA)[:npos]
            l = np.minimum(LA, r - np.arange(npos))
            d = ((win != A) & (np.arange(LA)[None, :] < l[:, None])).sum(axis=1)
            hit = np.flatnonzero(d <= al[l])
            if len(hit) and (best < 0 or hit[0] < best):
                best = int(hit[0])
        if best >= 0:
            cuts[i] = s1 + best
    return cuts, s1s


def truncate(reads, quals, cuts):
    """the reads and quality lines cut to cuts[i] letters (-1: as they are); a read cut to nothing is written as N / !"""
    out_r, out_q = [], []
    for r, q, c in zip(reads, quals, cuts):
        r, q, c = bytes(r), bytes(q), int(c)
        if c < 0:
            out_r.append(r)
            out_q.append(q)
        elif c == 0:
            out_r.append(b"N")
            out_q.append(b"!")
        else:
            out_r.append(r[:c])
            out_q.append(q[:c])
    return out_r, out_q


def record_counts(reads, cuts, s1, k):
    """what bk_adapter_stats reports -- [reads cut, bases removed] -- counted on the records: a last run of valid letters shorter
    than k makes no record (it holds no k-mer, cut or not) and is not counted"""
    n_cut = removed = 0
    for r, c, s in zip(reads, cuts, s1):
        if c >= 0 and len(r) - int(s) >= k:
            n_cut += 1
            removed += len(r) - int(c)
    return [n_cut, removed]


def emptied(reads, cuts, s1, k):
    """(records, bases): the last runs that held a record and are left with fewer than k letters by the cut"""
    left = [int(c) - int(s) for r, c, s in zip(reads, cuts, s1) if c >= 0 and len(r) - int(s) >= k and int(c) - int(s) < k]
    return len(left), sum(left)


def hamming_at_cut(read, cut, s1, adapters, E):
    """[(distance, allowance)] per adapter at the read's cut position"""
    R = bytes(read)[int(s1):].upper()
    p = int(cut) - int(s1)
    out = []
    for A in adapters:
        A = bytes(A).upper()
        l = min(len(A), len(R) - p)
        out.append((primer_ref.hamming(R[p:p + l], A[:l]), allowed(E, l)))
    return out


def masked(reads, quals, min_qual):
    """the reads with every base whose quality is below min_qual written as N (min_qual 0: as they are)"""
    if not min_qual:
        return reads
    out = []
    for r, ql in zip(reads, quals):
        a = np.frombuffer(r, np.uint8).copy()
        a[np.frombuffer(ql, np.uint8) < 33 + min_qual] = ord("N")
        out.append(a.tobytes())
    return out


def seen_reads(reads, quals, adapters, O, E, k, min_qual, primers=None, m=1):
    """(the reads every result is defined by, adapter counters, primer counters or None, the share of reads cut): truncate, then mask,
    then substitute"""
    cuts, s1 = cut_positions_all(reads, adapters, O, E, quals, min_qual)
    trunc, tq = truncate(reads, quals, cuts)
    want = masked(trunc, tq, min_qual)
    pcounts = None
    if primers:
        p5, p3, e0, ps1 = primer_ref.trim_lengths_all(trunc, primers, m, tq, min_qual)
        want = primer_ref.substitute(want, p5, p3, e0)
        pcounts = primer_ref.record_counts(trunc, p5, p3, e0, ps1, k)
    return want, record_counts(reads, cuts, s1, k), pcounts, (cuts >= 0).mean()


# ---- reads ------------------------------------------------------------------------------------------------------------------------
def _tail(rng, n, poly_g):
    return b"G" * n if poly_g else np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def read_through(insert, adapter, read_len, rng, poly_g):
    """the first read_len letters of insert + adapter + (poly-G or random) tail"""
    s = bytes(insert) + bytes(adapter)
    if len(s) < read_len:
        s += _tail(rng, read_len - len(s), poly_g)
    return s[:read_len]


def library_reads(sample, amps, adapters, n_reads, read_len, seed, short=0.45, amplicon=0.4, err=0.004):
    """Shotgun and amplicon reads of `sample`.  About `short` of the shotgun inserts are shorter than the read (uniform from 0 --
    an adapter dimer -- to read_len - 1, so that every partial adapter length occurs at the read end) and run on into an adapter
    and a poly-G or random tail; amplicon reads (from either strand, the primer stretches overwritten with the primers) of an
    amplicon shorter than the read do the same, the reverse-complemented far primer right before the adapter.  Sequencing
    errors everywhere, the adapter included."""
    rng = np.random.default_rng(seed)
    sample = bytes(sample)
    short_amps = [a for a in amps if a[1] - a[0] < read_len]
    out = []
    for i in range(n_reads):
        A = adapters[int(rng.integers(0, len(adapters)))]
        poly_g = bool(rng.random() < 0.5)
        if amps and rng.random() < amplicon:
            pool = short_amps if (short_amps and rng.random() < 0.6) else amps
            a, b, fwd, rev = pool[int(rng.integers(0, len(pool)))]
            amp = fwd + sample[a + len(fwd):b - len(rev)] + primer_ref.revcomp(rev)
            if rng.random() < 0.5:
                amp = primer_ref.revcomp(amp)
            r = read_through(amp, A, read_len, rng, poly_g) if len(amp) < read_len else amp[:read_len]
        else:
            ins = int(rng.integers(0, read_len)) if rng.random() < short else read_len
            p = int(rng.integers(0, len(sample) - read_len))
            frag = sample[p:p + ins]
            if rng.random() < 0.5:
                frag = primer_ref.revcomp(frag)
            r = read_through(frag, A, read_len, rng, poly_g)
        hits = [int(p) for p in np.flatnonzero(rng.random(len(r)) < err)]
        out.append(primer_ref.mutate(r, hits, rng) if hits else r)
    return out


def edge_reads(genome, adapters, O, E, read_len, seed):
    """[(read, tag)]: the edge cases, each with a word that says what it was built as"""
    rng = np.random.default_rng(seed)
    genome = bytes(genome)
    out = []
    at = [1000]

    def body(n):
        at[0] = (at[0] + 211) % (len(genome) - 400)
        return genome[at[0]:at[0] + n]
    for A in adapters:
        A = bytes(A)
        LA = len(A)
        for l in range(O - 1, LA + 1):                                 # a partial adapter of every length at the read's end
            out.append((body(read_len - l) + A[:l], "partial %d" % l))
        out.append((read_through(b"", A, read_len, rng, True), "dimer"))
        out.append((read_through(b"", A, read_len, rng, False), "dimer"))
        out.append((A, "dimer"))                                       # the adapter alone
        m = allowed(E, LA)
        spots = [int(x) for x in np.linspace(1, LA - 1, m + 1).astype(int)]   # m + 1 distinct places (LA >= 8, m <= 19)
        assert len(set(spots)) == m + 1
        for j in range(4):
            head = body(20 + 13 * j)
            rest = read_len - len(head) - LA
            out.append((head + primer_ref.mutate(A, spots[:m], rng) + _tail(rng, max(rest, 0), j % 2 == 0), "at the allowance"))
            out.append((head + primer_ref.mutate(A, spots, rng) + _tail(rng, max(rest, 0), j % 2 == 0), "near miss"))
        out.append((body(40) + A[:5] + b"N" + A[6:] + _tail(rng, 30, False), "N inside"))
        out.append((body(40) + A + body(20) + b"N" + body(30), "before an N"))
        out.append(((body(60) + A + _tail(rng, 20, True)).lower(), "lower case"))
        out.append((body(30).lower() + A.lower()[:LA // 2] + A[LA // 2:], "lower case"))
        out.append((body(10), "short"))
        out.append((body(25) + A[:O], "partial %d" % O))
    return out


def long_reads(genome, adapters, seed):
    """[(read, tag)]: records of more than 20,000 bases with an adapter deep inside, one behind an N, one run longer than a record
    holds (untrimmed), and a few ordinary reads around them"""
    rng = np.random.default_rng(seed)
    genome = bytes(genome)
    A = bytes(adapters[0])
    big = genome * (70000 // len(genome) + 2)
    out = [(big[37:37 + 15001] + A + _tail(rng, 5100, False), "deep"),
           (big[100:100 + 3000] + b"N" + big[500:500 + 19000] + A[:len(A) - 1], "deep"),
           (big[11:11 + 8000] + A + big[900:900 + 2000] + b"N" + big[5:5 + 12000], "before an N"),
           (_tail(rng, 30000, False) + A + _tail(rng, 40000, False), "too long"),
           (big[:66000] + A, "too long")]
    for j in range(12):
        out.append((genome[500 * j:500 * j + 100 + j] + A + _tail(rng, 40 - j, j % 2 == 0), "plain"))
        out.append((genome[300 * j:300 * j + 150], "plain"))
    return out
