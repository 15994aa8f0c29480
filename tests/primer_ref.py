"""The contract of --primers restated in Python (tests only): valid letters, the trim lengths p5 / p3, the N-substituted reads every
result is defined by, the end flags the packers give their records, and amplicon reads to try it all on."""
import numpy as np

MAXB = 65520   # bases of the longest record (4095 words): a longer run of valid letters is cut into chunks and its ends are not trimmed

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def valid(read, qual=None, min_qual=0):
    """which letters are valid: ACGT/acgt and, with min_qual > 0, a quality byte of '!' + min_qual or more"""
    a = np.frombuffer(bytes(read), np.uint8)
    v = np.isin(a & 0xDF, np.frombuffer(b"ACGT", np.uint8)) & np.isin(a, np.frombuffer(b"ACGTacgt", np.uint8))
    if qual is not None and min_qual > 0:
        v &= np.frombuffer(bytes(qual), np.uint8) >= 33 + min_qual
    return v


def end_runs(read, qual=None, min_qual=0):
    """(e0, s1): the end of the maximal valid prefix, the start of the maximal valid suffix"""
    v = valid(read, qual, min_qual)
    n = len(v)
    bad = np.flatnonzero(~v)
    if len(bad) == 0:
        return n, 0
    return int(bad[0]), int(bad[-1]) + 1


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


def trim_lengths(read, primers, m, qual=None, min_qual=0, maxb=MAXB):
    """(p5, p3) of one read, letter by letter as the contract states it"""
    read = bytes(read)
    n = len(read)
    e0, s1 = end_runs(read, qual, min_qual)
    up = read.upper()
    p5 = p3 = 0
    for p in primers:
        p = bytes(p).upper()
        L = len(p)
        if L <= e0 <= maxb and L > p5 and hamming(up[:L], p) <= m:
            p5 = L
        if L <= n - s1 <= maxb and L > p3 and hamming(up[n - L:], revcomp(p)) <= m:
            p3 = L
    return p5, p3


def trim_lengths_all(reads, primers, m, quals=None, min_qual=0):
    """trim_lengths for many reads at once (numpy over the reads, primer by primer): arrays p5, p3, e0, s1"""
    reads = [bytes(r) for r in reads]
    n_r = len(reads)
    lens = np.array([len(r) for r in reads], np.int64)
    width = max(int(lens.max()) if n_r else 0, 64)
    left = np.zeros((n_r, width), np.uint8)    # read i from column 0
    right = np.zeros((n_r, width), np.uint8)   # read i ending at the last column
    e0 = np.zeros(n_r, np.int64)
    s1 = np.zeros(n_r, np.int64)
    for i, r in enumerate(reads):
        a = np.frombuffer(r.upper(), np.uint8)
        left[i, :len(a)] = a
        if len(a):
            right[i, width - len(a):] = a
        e0[i], s1[i] = end_runs(r, None if quals is None else quals[i], min_qual)
    p5 = np.zeros(n_r, np.int64)
    p3 = np.zeros(n_r, np.int64)
    for p in primers:
        p = np.frombuffer(bytes(p).upper(), np.uint8)
        rc = np.frombuffer(revcomp(bytes(p)), np.uint8)
        L = len(p)
        d5 = (left[:, :L] != p).sum(axis=1)
        d3 = (right[:, width - L:] != rc).sum(axis=1)
        ok5 = (d5 <= m) & (L <= e0) & (e0 <= MAXB)
        ok3 = (d3 <= m) & (L <= lens - s1) & (lens - s1 <= MAXB)
        p5 = np.where(ok5, np.maximum(p5, L), p5)
        p3 = np.where(ok3, np.maximum(p3, L), p3)
    return p5, p3, e0, s1


def substitute(reads, p5, p3, e0):
    """the reads with the letters [0, p5) and [n - p3, n) replaced by N (the whole read if it is one run and they meet)"""
    out = []
    for r, a, b, e in zip(reads, p5, p3, e0):
        r = bytes(r)
        n = len(r)
        if e == n and a + b >= n and (a or b):
            out.append(b"N" * n)
        else:
            out.append(b"N" * int(a) + r[int(a):n - int(b)] + b"N" * int(b))
    return out


def trimmed(reads, primers, m, quals=None, min_qual=0):
    p5, p3, e0, _ = trim_lengths_all(reads, primers, m, quals, min_qual)
    return substitute(reads, p5, p3, e0)


def record_counts(reads, p5, p3, e0, s1, k):
    """what bk_primer_stats reports -- [reads trimmed at 5', reads trimmed at 3', bases masked] -- counted on the records: an end
    whose run of valid letters is shorter than k makes no record (it holds no k-mer either way) and is not counted"""
    t5 = t3 = masked = 0
    for r, a, b, e, s in zip(reads, p5, p3, e0, s1):
        n = len(r)
        a = int(a) if e >= k else 0
        b = int(b) if n - s >= k else 0
        t5 += a > 0
        t3 += b > 0
        masked += min(n, a + b) if e == n else a + b
    return [t5, t3, masked]


def end_flags(reads, k, stride_words=None, quals=None, min_qual=0):
    """(bases, flags) of every record the packers make of the reads, in order: one record per maximal run of at least k valid
    letters (bit 0: the run starts the read, bit 1: it ends the read), a run longer than a record cut into chunks that overlap by
    k - 1 and carry no flag"""
    if stride_words is None:
        stride_words = min((max([len(r) for r in reads] + [k]) + 15) // 16, 4095)
    maxb = min(stride_words * 16, 65535)
    out = []
    for i, r in enumerate(reads):
        r = bytes(r)
        v = valid(r, None if quals is None else quals[i], min_qual)
        n = len(r)
        start = 0
        for p in range(n + 1):
            if p < n and v[p]:
                continue
            run = p - start
            if run >= k:
                fl = ((1 if start == 0 else 0) | (2 if p == n else 0)) if run <= maxb else 0
                pos = 0
                while True:
                    take = min(maxb, run - pos)
                    out.append((r[start + pos:start + pos + take].upper(), fl))
                    if pos + take >= run:
                        break
                    pos += take - (k - 1)
            start = p + 1
    return out


# ---- amplicon reads ---------------------------------------------------------------------------------------------------------------
def tile_amplicons(ref, seed, special=(12, 31, 32, 33, 64)):
    """The genome tiled with overlapping amplicons: about three quarters ~400 bp, a quarter 90..140 bp (shorter than a 150-base
    read: it runs into the far primer's reverse complement).  Primers of 18..32 bases cut from the amplicon ends, a few of the
    `special` lengths.  Returns [(start, end, fwd_primer, rev_primer)] -- the reverse primer as synthesised (the reverse complement
    of the amplicon's last bases)."""
    rng = np.random.default_rng(seed)
    amps = []
    at = 0
    i = 0
    while at + 500 < len(ref):
        ln = int(rng.integers(90, 141)) if i % 4 == 3 else int(rng.integers(380, 421))
        lf, lr = int(rng.integers(18, 33)), int(rng.integers(18, 33))
        if i < 2 * len(special):
            if i % 2 == 0:
                lf = special[i // 2]
            else:
                lr = special[i // 2]
        ln = max(ln, lf + lr + 8)
        a, b = at, at + ln
        amps.append((a, b, bytes(ref[a:a + lf]), revcomp(ref[b - lr:b])))
        at = b - int(rng.integers(60, 90)) if ln > 200 else b - 40   # (neighbours overlap: a primer site lies inside the next amplicon)
        at = max(at, a + 30)
        i += 1
    return amps


def mutate(s, positions, rng):
    a = bytearray(s)
    for p in positions:
        a[p] = b"ACGT"[(b"ACGT".index(bytes([a[p]]).upper()) + int(rng.integers(1, 4))) & 3]
    return bytes(a)


def amplicon_reads(ref, sample, amps, n_reads, read_len, seed, shotgun=0.2, bad_primer=0.1, err=0.005):
    """n_reads reads of `sample` (the sample's genome, as long as `ref`): about 80 % amplicon reads from either strand, whose primer
    stretches are overwritten with the primers themselves (they carry the reference base), about 20 % shotgun reads; about 10 %
    of the amplicon reads with two or three mismatches in their 5' primer, some with exactly one at the primer's first, last and
    word-boundary positions; sequencing errors elsewhere."""
    rng = np.random.default_rng(seed)
    ref, sample = bytes(ref), bytes(sample)
    out = []
    for i in range(n_reads):
        if rng.random() < shotgun:
            p = int(rng.integers(0, len(sample) - read_len))
            r = sample[p:p + read_len]
            if rng.random() < 0.5:
                r = revcomp(r)
        else:
            a, b, fwd, rev = amps[int(rng.integers(0, len(amps)))]
            amp = fwd + sample[a + len(fwd):b - len(rev)] + revcomp(rev)
            lead = fwd
            if rng.random() < 0.5:
                amp = revcomp(amp)
                lead = rev
            r = amp[:read_len]
            L = min(len(lead), len(r))
            u = rng.random()
            if u < bad_primer:
                r = mutate(r, rng.choice(L, size=int(rng.integers(2, 4)), replace=False), rng)
            elif u < bad_primer + 0.12:
                r = mutate(r, [[0, L - 1, min(15, L - 1), min(16, L - 1)][i % 4]], rng)
        body = np.flatnonzero(rng.random(len(r)) < err)
        body = [int(p) for p in body if 40 <= p < len(r) - 70]   # (errors away from the primer stretches: those are counted above)
        out.append(mutate(r, body, rng) if body else r)
    return out


def edge_reads(ref, amps, read_len):
    """the edge cases: an N inside the primer, lower case, a read shorter than its primer, a read equal to a primer, primer dimers,
    an N right behind a primer, an internal primer"""
    ref = bytes(ref)
    out = []
    for j, (a, b, fwd, rev) in enumerate(amps[:24]):
        amp = fwd + ref[a + len(fwd):b - len(rev)] + revcomp(rev)
        r = amp[:read_len]
        out.append(r[:5] + b"N" + r[6:])                      # an N inside the primer
        out.append(r.lower())
        out.append(fwd[:-1])                                  # shorter than its primer
        out.append(fwd)                                       # equal to a primer: the whole read is masked
        out.append(rev)
        other = amps[(j + 7) % len(amps)][3]
        out.append(fwd + revcomp(other))                      # a primer dimer: p5 + p3 = n
        out.append(fwd + revcomp(other)[4:])                  # ... overlapping
        out.append(fwd + b"N" + r[len(fwd) + 1:])             # an N right behind the primer: the 5' run is the primer alone
        out.append(ref[a + 50:a + 70] + fwd + ref[a + 70:a + 150])   # an internal primer: no match
        out.append(r[:len(r) - 3] + b"NNN")                   # the read's end masked
        out.append(revcomp(amp)[:read_len].lower())
    return out
