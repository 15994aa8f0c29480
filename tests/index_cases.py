"""Cases for the index builders -- bk_build_index on the device (bronko_amd/csrc/bk_build.hip), the host's build_indexes_mem and the
oracle's -- and a plain reference of what they must make of them.

expected(k, files) is build.rs:145-231 over oracle/cross_oracle.py's literal restatement of lcb.rs (canonical_kmer, assign_buckets:
Python integers masked to 64 bits, a dictionary of lists), with the project's one rule on top: a sequence shorter than k adds
nothing and still takes its seq_id (upstream panics there, and so does cross_oracle.build_indexes_files).  It returns
(bucket_ids, bucket_off, entries): the buckets in ascending id, every list in (file, sequence, location, idx) order of generation,
the entries in a zero-filled array of the 12-byte BucketInfo, so that the padding bytes can be compared as well.

make_case(seed, iteration) draws one case from numpy's generator seeded with (seed, iteration); nothing else goes in.
named_cases() are the hand-made ones: every odd k, every byte value, the lengths around k at every place, 256 sequences in a file,
buckets far longer than a chunk of the device build's host tail, locations beyond 2^16, forty identical files.  tally() counts
what a run of fuzz cases has reached, for the conditions of tests/test_index_cases_cpu.py.  tests/test_gpu_index_fuzz.py runs the
same cases through build_index_device.

Everything here is plain Python and numpy; no product code is imported.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import cross_oracle

SEED = 20264                                     # the suite's seed
BLOCK, BLOCKS = 30, 4                            # the suite's iterations: BLOCKS blocks of BLOCK
KS = tuple(range(3, 32, 2)) + (21, 31)           # every odd k; 21 and 31 twice as likely
MAX_PAIRS = 60000                                # a fuzz case stays below: expected() takes under a second
CHUNK = 65536                                    # the device build's host tail cuts about so many pairs per thread

# BucketInfo (build.rs:52-60, #[repr(C)]): u16 file_id, u8 seq_id, (1 byte), u32 location, u8 idx, bool canonical, (2 bytes)
BUCKET_INFO_DTYPE = np.dtype({"names": ["file_id", "seq_id", "location", "idx", "canonical"],
                              "formats": [np.uint16, np.uint8, np.uint32, np.uint8, np.uint8],
                              "offsets": [0, 2, 4, 8, 9], "itemsize": 12})

ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
# what stands in a sequence beside ACGT: N, the IUPAC letters, gap and stop signs, bytes at or above 0x80 (never a line break or '>':
# the cases are also written as FASTA files)
OTHER = b"NnRYKMSWBDHVrykmswbdhvUu-*." + bytes([0x80, 0x81, 0xC1, 0xE7, 0xFE, 0xFF])


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n: int) -> bytes:
    return bytes(ACGT[i] for i in rng.integers(0, 4, n))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _walk(k: int, files):
    """build.rs:191-204 for every sequence of at least k symbols: (bucket id -> [(file_id, seq_id, location, idx, canonical)]) in the
    order of generation, and the canonical k-mers met"""
    index, memo = {}, {}
    for f, (_, records) in enumerate(files):
        for s, (_, seq) in enumerate(records):               # seq_id counts every record (build.rs:170, :207)
            seq = bytes(seq)
            if len(seq) < k:                                 # the project's rule; upstream would panic
                continue
            for i in range(len(seq) - k + 1):
                key = cross_oracle.canonical_kmer(seq[i:i + k], k)
                if key not in memo:
                    memo[key] = cross_oracle.assign_buckets(key[0], k)
                c = int(key[1])
                for j, b in enumerate(memo[key]):
                    index.setdefault(b, []).append((f, s, i, j, c))
    return index, memo


def _flatten(index):
    ids = sorted(index)
    off = np.zeros(len(ids) + 1, np.uint64)
    rows = []
    for n, b in enumerate(ids):
        rows += index[b]
        off[n + 1] = len(rows)
    ent = np.zeros(len(rows), BUCKET_INFO_DTYPE)             # (zero-filled: the padding bytes are compared)
    if rows:
        a = np.array(rows, np.int64)
        for c, name in enumerate(BUCKET_INFO_DTYPE.names):
            ent[name] = a[:, c]
    return np.array(ids, np.uint64), off, ent


def expected(k: int, files):
    """(bucket_ids u64[n], bucket_off u64[n + 1], entries BucketInfo[m]) of the index of `files` = [(file name, [(sequence name,
    sequence bytes)])]"""
    return _flatten(_walk(k, files)[0])


def n_pairs(k: int, files) -> int:
    return sum(len(s) - k + 1 for _, recs in files for _, s in recs if len(s) >= k) * k


# ---- the fuzz ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str                        # "fuzz" or a named case's name
    seed: int
    it: int
    k: int
    files: list                      # [(file name, [(sequence name, bytes)])]
    notes: str = ""                  # what the generator laid into it

    def describe(self) -> str:
        return "%s seed=%d it=%d k=%d files=%d seqs=%s pairs=%d %s" % (
            self.name, self.seed, self.it, self.k, len(self.files), [[len(s) for _, s in recs] for _, recs in self.files][:12],
            n_pairs(self.k, self.files), self.notes)


def _run(rng) -> bytes:
    """a homopolymer or dinucleotide run of 50 to 2,000 bases"""
    unit = rand_seq(rng, int(rng.integers(1, 3)))
    n = int(rng.integers(50, 2001))
    return (unit * n)[:n]


def _dress(rng, seq: bytes, k: int, notes: set) -> bytes:
    """lower-case stretches and symbols outside ACGT: at the first, the last and the k-th place as well as inside"""
    s = bytearray(seq)
    n = len(s)
    if n and rng.random() < 0.25:
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(1, 200)))
            s[a:b] = bytes(s[a:b]).lower()
        notes.add("lower")
    if n and rng.random() < 0.35:
        places = set()
        for _ in range(int(rng.integers(1, 6))):
            u = rng.random()
            places.add(0 if u < 0.15 else n - 1 if u < 0.3 else min(n - 1, k - 1) if u < 0.4 else min(n - 1, k) if u < 0.5 else int(rng.integers(0, n)))
        if rng.random() < 0.3:                               # a run of them
            a = int(rng.integers(0, n))
            places |= set(range(a, min(n, a + int(rng.integers(2, 40)))))
        for p in places:
            s[p] = OTHER[int(rng.integers(0, len(OTHER)))]
        notes.add("other")
    return bytes(s)


def make_case(seed: int, it: int) -> Case:
    """Case `it` of `seed`: k, one to eight files of zero to six sequences; lengths of {0, 1, k - 1, k, k + 1, 2k - 1} and of 30 to
    3,000; runs; copies of earlier files' sequences -- exact, with substitutions, reverse-complemented; lower case and other symbols.
    The case stays under MAX_PAIRS pairs: a sequence is cut to half of the k-mers the case may still take, to k - 1 bases once
    that is nothing."""
    rng = np.random.default_rng((seed, it))
    k = int(rng.choice(KS))
    left = MAX_PAIRS // k - 1                                # k-mers the case may still take
    notes = set()
    barren = rng.random() < 0.04                             # nothing to index at all
    if barren:
        notes.add("barren")
    n_files = int(rng.integers(1, 9))
    pool, files = [], []                                     # pool: (file, undressed sequence) of every sequence so far
    for f in range(n_files):
        recs = []
        for s in range(int(rng.integers(0, 7))):
            u = rng.random()
            others = [q for g, q in pool if g != f and len(q) >= k]
            if barren:
                seq = rand_seq(rng, int(rng.choice([0, 1, k - 1])))
            elif others and u < 0.4:                         # a copy of a sequence of another file
                seq = others[int(rng.integers(0, len(others)))]
                v = rng.random()
                if v < 0.35:
                    notes.add("copy")
                elif v < 0.65:
                    b = bytearray(seq)
                    for p in rng.integers(0, len(b), int(rng.integers(1, 6))):
                        b[p] = ACGT[(ACGT.index(b[p]) + int(rng.integers(1, 4))) & 3]
                    seq = bytes(b)
                    notes.add("copy_subst")
                else:
                    seq = revcomp(seq)
                    notes.add("copy_rc")
            elif u < 0.65:
                seq = rand_seq(rng, int(rng.choice([0, 1, k - 1, k, k + 1, 2 * k - 1])))
            else:
                seq = rand_seq(rng, int(rng.integers(30, 3001)))
                if rng.random() < 0.35:
                    run = _run(rng)
                    a = int(rng.integers(0, len(seq) + 1))
                    seq = run if rng.random() < 0.3 else seq[:a] + run + seq[a + len(run):]
                    notes.add("run")
            if len(seq) >= k and len(seq) - k + 1 > (left + 1) // 2:   # the budget: no more than half of what is left, or nothing to index
                seq = seq[:(left + 1) // 2 + k - 1] if left > 0 else seq[:k - 1]
            if len(seq) >= k:
                left -= len(seq) - k + 1
            pool.append((f, seq))
            recs.append(("s%d_%d" % (f, s), _dress(rng, seq, k, notes)))
        files.append(("file%d" % f, recs))
    return Case("fuzz", seed, it, k, files, ",".join(sorted(notes)))


# ---- the named cases --------------------------------------------------------------------------------------------------------------
def _named_rng(tag: int):
    return np.random.default_rng((SEED, 1000003, tag))


def lengths_files(k: int, rng):
    """Sequences of k - 1, k and k + 1 bases as the first, a middle and the last sequence of the first, a middle and the last file
    (each file begins with another of the three); between them a file of sequences shorter than k only and a file without sequences"""
    def file(name, order):
        a, b, c = [rand_seq(rng, k + d) for d in order]
        return (name, [("a", a), ("r0", rand_seq(rng, 60 + k)), ("b", b), ("r1", rand_seq(rng, 70)), ("c", c)])
    return [file("first", (-1, 0, 1)),
            ("shorts", [("t%d" % i, rand_seq(rng, n)) for i, n in enumerate((k - 1, 0, 1, k - 1, 2))]),
            ("plain0", [("p", rand_seq(rng, 90))]),
            file("middle", (0, 1, -1)),
            ("none", []),
            ("plain1", [("p", rand_seq(rng, 80))]),
            file("last", (1, -1, 0))]


def many_sequences_files(k: int, n: int, rng):
    """One file of n sequences whose lengths cycle through k, 40 and k - 1 (the 256th, seq_id 255, has k bases) and a second file"""
    lens = (k, 40, k - 1)
    return [("many", [("q%d" % i, rand_seq(rng, lens[i % 3])) for i in range(n)]), ("after", [("z", rand_seq(rng, 100))])]


def named_cases() -> list:
    """[Case]: the hand-made cases, the large ones included (see n_pairs)"""
    out = []

    def add(name, k, files, notes=""):
        out.append(Case(name, SEED, -1, k, files, notes))
    for k in range(3, 32, 2):
        g = rand_seq(_named_rng(k), 400)
        add("every_k[%d]" % k, k, [("fwd", [("g", g)]), ("rev", [("g_rc", revcomp(g))])])
    rng = _named_rng(100)
    add("every_byte", 11, [("bytes", [("b", rand_seq(rng, 60) + bytes(range(256)) + rand_seq(rng, 60))])])
    for k in (3, 21, 31):
        add("lengths[%d]" % k, k, lengths_files(k, _named_rng(200 + k)))
    add("many_sequences", 21, many_sequences_files(21, 256, _named_rng(300)))
    add("long_bucket", 11, [("poly", [("a", b"A" * 140010)]), ("rand", [("r", rand_seq(_named_rng(400), 500))])])
    add("deep_location", 15, [("periodic", [("p", (rand_seq(_named_rng(500), 997) * 71)[:70000])])])
    rng = _named_rng(600)
    three = [("x", rand_seq(rng, 60)), ("short", rand_seq(rng, 20)), ("y", rand_seq(rng, 45))]
    add("identical_files", 21, [("same%d" % f, list(three)) for f in range(40)])
    return out


# ---- what a run of fuzz cases reaches -----------------------------------------------------------------------------------------------
def lcb_rank_wraps(v: int, k: int, rank) -> bool:
    """whether one of the k exact ranks of canonical k-mer v (rank = tests.helpers.lcb_rank) is 2^64 or more"""
    return any(rank(v & ~(3 << (2 * (k - 1 - j))), j, k) >= 1 << 64 for j in range(k))


def reference(case: Case):
    """(expected(case.k, case.files), what tally() needs of the same walk)"""
    walked = _walk(case.k, case.files)
    return _flatten(walked[0]), walked


def tally(case: Case, into: dict, rank, walked=None) -> dict:
    """What the case reaches, from the reference alone (`walked`: reference(case)[1], where it is at hand), added into `into`"""
    def add(name, v=1):
        into[name] = into.get(name, 0) + int(v)
    k = case.k
    index, memo = walked if walked is not None else _walk(k, case.files)
    add("iterations")
    add("k=%d" % k)
    add("pairs", sum(len(v) for v in index.values()))
    add("buckets", len(index))
    if k == 31 and memo:
        add("it_k31_rank_wraps", lcb_rank_wraps(max(v for v, _ in memo), k, rank))
    add("buckets_200_entries_3_files", sum(1 for v in index.values() if len(v) >= 200 and len({e[0] for e in v}) >= 3))
    add("longest_bucket", 0)
    into["longest_bucket"] = max(into["longest_bucket"], max([len(v) for v in index.values()] + [0]))
    for d in (-1, 0, 1):
        add("it_last_sequence_of_k%+d" % d, any(recs and len(recs[-1][1]) == k + d for _, recs in case.files))
    add("it_no_kmer", not index)
    both = 0
    for v in index.values():
        seen = {}
        for e in v:
            seen[e[2]] = seen.get(e[2], 0) | (1 << e[4])
        both += any(x == 3 for x in seen.values())
    add("buckets_location_under_both_canonical", both)
    add("it_empty_file", any(not recs for _, recs in case.files))
    add("it_file_of_shorts_between", any(case.files[f][1] and all(len(s) < k for _, s in case.files[f][1]) and
                                         any(len(s) >= k for g in range(f) for _, s in case.files[g][1]) and
                                         any(len(s) >= k for g in range(f + 1, len(case.files)) for _, s in case.files[g][1])
                                         for f in range(len(case.files))))
    add("max_seq_id", 0)
    into["max_seq_id"] = max(into["max_seq_id"], max([e[1] for v in index.values() for e in v] + [0]))
    for note in case.notes.split(","):
        if note:
            add("it_" + note)
    return into


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def same(got, want) -> str | None:
    """None where (ids, off, entries) `got` equals `want` -- ids, offsets, and the entries byte for byte -- else what differs first"""
    gi, go, ge = got
    wi, wo, we = want
    if len(gi) != len(wi) or not np.array_equal(gi, wi):
        n = min(len(gi), len(wi))
        bad = np.flatnonzero(np.asarray(gi[:n]) != np.asarray(wi[:n]))
        return "bucket ids: %d against %d, first difference at %s" % (len(gi), len(wi), bad[:1].tolist())
    if not np.array_equal(go, wo):
        bad = np.flatnonzero(np.asarray(go) != np.asarray(wo))
        return "bucket offsets differ first at bucket %d: %d against %d" % (bad[0], go[bad[0]], wo[bad[0]])
    if ge.dtype.itemsize != 12 or len(ge) != len(we):
        return "entries: %d of %d bytes against %d" % (len(ge), ge.dtype.itemsize, len(we))
    a = np.ascontiguousarray(ge).view(np.uint8).reshape(-1, 12)
    b = np.ascontiguousarray(we).view(np.uint8).reshape(-1, 12)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero((a != b).any(axis=1))[0])
        bucket = int(np.searchsorted(np.asarray(wo), i, side="right") - 1)
        return "entry %d (bucket %d, which begins at %d) is %s (bytes %s), not %s (bytes %s)" % (
            i, bucket, wo[bucket], ge[i], a[i].tolist(), we[i], b[i].tolist())
    return None
