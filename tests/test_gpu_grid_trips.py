"""More records in one push than one trip of the grid: the second and later trips of the grid-stride loops of indel_scan_kernel,
link_scan_kernel, link_count_kernel, the codon and the haplotype kernels, and the three paths of indel_scan_kernel's per-wave queue
that only a second trip reaches (the carry-over, the drain at 64 waiting records, the walk of what remains).

One push of ceil(2.5 x CUs x 8 x 256) records of 64 bases on HPV16 at k = 21: a list of P distinct records (P prime) repeated
cyclically, so that no wave meets the same mixture twice.  Every result is additive over the records, so what is expected is the
restatements' result of the P records times each record's multiplicity: the full list never goes through the restatements.  All
comparisons are exact."""
import os
import random
from collections import Counter

import numpy as np
import pytest

from bronko_amd import pack_reads
from bronko_amd.engine import link_rows as decode_rows
from bronko_amd.hostlib import HostIndex
from tests import codons_ref, haplotypes_ref, indel_cases, indels_ref, linkage_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, N_LEN = 21, 64                    # a record is 3k + 1 bases: four words
L, M = 32, 8                         # indels: max_len, max_mismatches; linkage: max_mismatches M as well
LO, HI = 1990, 2150                  # the placed records start in these cells: the sites and regions below lie under many of them
LDS_PAIRS, LDS_CODONS = 512, 16384   # kLinkLdsPairs, kCodonLdsCodons


def _alone(g, rec):
    """(the lone record's indel counters, its events, what linkage makes of it, its row)"""
    res = indels_ref.indel_events(g, [rec], L, M)
    what, row = linkage_ref.place(g, rec, M)
    return res.counters, res.events, what, row


def _draw(g, rng, kind):
    """One record of the kind, along or against the reference; the caller keeps it if the restatement agrees about the kind"""
    t = g.text
    start = rng.randrange(LO, HI)
    if kind == "del":
        d = rng.choice((1, 2, 3, 5, 8, 13, 21, 32))
        r = indel_cases.mut_read(t, start, N_LEN, dele=(start + rng.randrange(K, 2 * K + 2), d), subs=tuple(rng.sample(range(K), rng.choice((0, 0, 1)))))
    elif kind == "ins":
        i = rng.choice((1, 2, 3, 5, 8, 13, 18, 22))
        r = indel_cases.mut_read(t, start, N_LEN, ins=(start + rng.randrange(K, 2 * K + 2 - i + 1), indel_cases._rand(rng, i)))
    elif kind == "plain":
        r = t[start:start + N_LEN]
    elif kind.startswith("subs"):                                  # subsN: N substitutions, most between the anchors' first tries
        n = int(kind[4:])
        offs = rng.sample(range(K, 2 * K + 1), n)
        if n < 8 and rng.random() < 0.3:
            offs[0] = rng.choice((3, N_LEN - 4))                   # ... one in an end's first anchor k-mer: the second try places it
        r = indel_cases.mut_read(t, start, N_LEN, subs=tuple(offs))
    elif kind == "foreign":
        r = indel_cases._rand(rng, N_LEN)
    else:                                                          # two halves a hundred cells apart: |delta| = 100
        assert kind == "chimera"
        r = t[start:start + N_LEN // 2] + t[start + 100 + N_LEN // 2:start + 100 + N_LEN]
    return indels_ref.revcomp(r) if rng.random() < 0.5 else r


def _is(g, rec, kind):
    c, events, what, row = _alone(g, rec)
    if kind in ("del", "ins"):
        return c["supporting"] == 1 and what == "unplaced" and [e[1] for e in events] == [indels_ref.DEL if kind == "del" else indels_ref.INS]
    if kind == "plain":
        return c["ref_spanning"] == 1 and what == "placed" and row[3] == ()
    if kind == "subs9":
        return c["anchored"] == 1 and c["discordant"] == 1 and what == "discordant"
    if kind.startswith("subs"):
        return c["ref_spanning"] == 1 and what == "placed" and len(row[3]) == int(kind[4:])
    if kind == "foreign":
        return c["anchored"] == 0 and what == "unplaced"
    return c["anchored"] == 1 and c["discordant"] == 1 and what == "unplaced"   # chimera


def _records(g, mix):
    """(the P distinct records, which of them have delta != 0 and pass the checks -- the ones the indel kernel queues)"""
    rng = random.Random(31 if mix == "half" else 32)
    if mix == "half":                                              # P = 101: 40 queued, 56 placed by linkage, 5 neither
        slow = ["del", "ins"] * 20
        rest = ["plain"] * 18 + ["subs%d" % n for n in (1, 2, 3, 4, 5, 6, 7) for _ in range(4)] + ["subs8"] * 10 + ["subs9", "subs9", "foreign", "foreign", "chimera"]
    else:                                                          # P = 97: every record is queued
        slow, rest = ["del", "ins"] * 48 + ["del"], []
    rng.shuffle(slow)
    rng.shuffle(rest)
    n_slow, P = len(slow), len(slow) + len(rest)
    # the queued records are spread evenly through the list: any 64 consecutive records hold about 64 * n_slow / P of them
    kinds = [slow.pop() if (j + 1) * n_slow // P > j * n_slow // P else rest.pop() for j in range(P)]
    recs, seen = [], set()
    for kd in kinds:
        for _ in range(200):
            r = _draw(g, rng, kd)
            if r not in seen and _is(g, r, kd):
                break
        else:
            raise AssertionError("no record of kind %s" % kd)
        seen.add(r)
        recs.append(r)
    return recs, np.array([kd in ("del", "ins") for kd in kinds])


def _queue_walk(queued, n, grid):
    """indel_scan_kernel's queue as the host counts it from the list and the record order: a wave of workgroup b takes the records
    [256 b + 64 w + trip * 256 grid, + 64).  Returns per wave: what it queued on each trip, the trips at whose end it walked 64, how
    many waited when a trip began, what remained at the end."""
    waves = grid * 4
    trips = -(-n // (waves * 64))
    flags = np.zeros(trips * waves * 64, np.int64)
    flags[:n] = queued[np.arange(n) % len(queued)]
    per_trip = flags.reshape(trips, waves, 64).sum(axis=2)
    qn = np.zeros(waves, np.int64)
    drained, carried = np.zeros((trips, waves), bool), np.zeros((trips, waves), np.int64)
    for t in range(trips):
        carried[t] = np.where(per_trip[t] > 0, qn, 0)
        qn = qn + per_trip[t]
        drained[t] = qn >= 64
        qn = qn - 64 * drained[t]
        assert (qn < 64).all()
    return per_trip, drained, carried, qn


def _scaled(a, b, q):
    """q times the result of all P records plus once that of the first N mod P"""
    return q * np.asarray(a, np.int64) + np.asarray(b, np.int64)


def _unique_rows(raw):
    """{decoded row: how often} of an (n, 32) byte array, counted in numpy"""
    if len(raw) == 0:
        return {}
    w = np.ascontiguousarray(raw).view("<u8").reshape(-1, 4)
    order = np.lexsort((w[:, 3], w[:, 2], w[:, 1], w[:, 0]))
    s = w[order]
    first = np.concatenate([[True], (s[1:] != s[:-1]).any(axis=1)])
    at = np.flatnonzero(first)
    counts = np.diff(np.concatenate([at, [len(s)]]))
    out = {}
    for i, c in zip(at, counts):
        out[decode_rows(raw[order[i]][None, :])[0]] = int(c)
    assert len(out) == len(at)
    return out


@pytest.fixture(scope="module")
def world():
    ix = HostIndex.load(os.path.join(GOLDEN, "hpv.bkdb"))
    g = indels_ref.read_fasta(os.path.join(GOLDEN, "HPV16.fa"), K)
    eng = ix.engine()
    eng.indels_enable(L, M)
    eng.linkage_enable(M)
    yield ix, g, eng
    eng.close()
    ix.close()


@pytest.mark.parametrize("mix", ["half", "all"])
def test_two_and_a_half_trips_of_the_grid_in_one_push(world, mix):
    import torch
    ix, g, eng = world
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * 8
    n = -(-5 * grid * 256 // 2)                                    # ceil(2.5 x CUs x 8 x 256)
    recs, queued = _records(g, mix)
    P = len(recs)
    assert P in (97, 101) and len(set(recs)) == P and all(len(r) == N_LEN for r in recs)
    q, rem = divmod(n, P)

    # the queue's paths, counted on the host before anything is pushed
    per_trip, drained, carried, left = _queue_walk(queued, n, grid)
    trips, waves = per_trip.shape
    assert trips == 3 and waves == grid * 4
    full = np.arange(trips)[:, None] * waves * 64 + np.arange(waves)[None, :] * 64 + 64 <= n   # the trips that hold 64 records
    if mix == "half":
        assert 0.35 < queued.mean() < 0.55
        assert per_trip[full].min() >= 20 and per_trip[full].max() <= 45, (per_trip[full].min(), per_trip[full].max())
        three = full[2]                                            # the waves that go round three times
        assert three.sum() >= waves // 4 and not drained[0].any()
        assert (drained[1, three] | drained[2, three]).all()       # ... cross 64 on their second or third trip
        assert (carried[1] > 0).all() and (carried[2, three] > 0).all()   # every later trip begins with records waiting
        assert (left > 0).all()                                    # every wave walks a remainder at the end
    else:
        assert queued.all() and (per_trip[full] == 64).all() and full.sum() * 64 == n
        assert (drained == full).all() and (carried == 0).all() and (left == 0).all()   # every trip of every wave drains at exactly 64

    words, lens = pack_reads([r.encode() for r in recs], K)
    assert words.shape == (P, 4) and (lens == N_LEN).all()
    idx = np.arange(n) % P
    eng.sample_begin()
    eng.push_reads(0, words[idx], lens[idx])
    eng.sample_finalize(1)

    # indels: events per strand, span, counters
    a, b = indels_ref.indel_events(g, recs, L, M), indels_ref.indel_events(g, recs[:rem], L, M)
    both = indels_ref.Result({key: [q * f + b.events.get(key, [0, 0])[0], q * r + b.events.get(key, [0, 0])[1]] for key, (f, r) in a.events.items()},
                             _scaled(a.span, b.span, q).tolist(), {name: q * a.counters[name] + b.counters[name] for name in a.counters})
    assert set(b.events) <= set(a.events) and len(a.events) >= (30 if mix == "half" else 80)
    eng.sample_indels(1, 0)
    summ, rows = eng.download_indels()
    want = indels_ref.table_rows(g, both)
    assert rows == want, ([r for r in rows if r not in want][:3], [r for r in want if r not in rows][:3])
    c = both.counters
    assert (summ.records, summ.anchored, summ.ref_spanning, summ.supporting, summ.discordant) == \
        (c["records"], c["anchored"], c["ref_spanning"], c["supporting"], c["discordant"]) and c["records"] == n
    assert summ.candidates == summ.reported == len(want) and summ.overflow == 0
    assert c["supporting"] == int(queued[idx].sum())
    span = eng.download_indel_span()
    sums = np.array(both.span_sums()[:g.cells], np.int64).astype(np.uint32)
    assert np.array_equal(span, sums), np.flatnonzero(span != sums)[:5]

    # the row store as a multiset, in numpy; the tallies
    placed = [linkage_ref.place(g, r, M) for r in recs]
    mult = [q + (1 if i < rem else 0) for i in range(P)]
    want_rows, tallies = Counter(), Counter()
    for (what, row), m in zip(placed, mult):
        tallies[what] += m
        if row is not None:
            want_rows[row] += m
    raw = eng.download_link_rows(raw=True)
    assert raw.shape == (tallies["placed"], 32) and raw.dtype == np.uint8
    print("%s: %d CUs, %d records in one push, %d rows in the store" % (mix, cus, n, len(raw)))
    assert _unique_rows(raw) == dict(want_rows)
    rows_all = [row for _, row in placed if row is not None]
    rows_rem = [row for _, row in placed[:rem] if row is not None]
    if mix == "half":
        assert tallies["placed"] >= 0.54 * n and tallies["discordant"] > 0   # 0.7 M rows on 256 CUs: five and a half trips at two workgroups a CU
        assert len(set(rows_all)) == len(rows_all) and {r[2] for r in rows_all} == {0, 1} and max(len(r[3]) for r in rows_all) == 8
    else:
        assert tallies["placed"] == 0 and tallies["unplaced"] == n

    def pairs_of(sites):
        one, two = linkage_ref.link_count(g, rows_all, sites, 1000), linkage_ref.link_count(g, rows_rem, sites, 1000)
        return [(x[0], x[1], _scaled(x[2], y[2], q).tolist()) for x, y in zip(one, two)]

    few, many = [2040, 2044, 2051, 2052, 2060], list(range(2030, 2075))
    for sites in (few, many):                                      # the LDS kernel, then the global-atomic kernel
        want = pairs_of(sites)
        assert (len(want) <= LDS_PAIRS) == (sites is few)
        eng.sample_linkage(sites, 1000)
        summ, pairs = eng.download_linkage()
        assert (summ.records, summ.placed, summ.unplaced, summ.discordant) == (n, tallies["placed"], tallies["unplaced"], tallies["discordant"])
        assert (summ.n_sites, summ.n_pairs) == (len(sites), len(want)) and pairs == want, [x for x in zip(pairs, want) if x[0] != x[1]][:2]
        assert mix == "all" or sum(sum(cnt) for _, _, cnt in want) > n // 4

    # codons: a few (the difference array in LDS), then more than kCodonLdsCodons (global atomics)
    cells = g.cells
    for regions in ([(2000 + f, 60) for f in range(3)], [(f, (cells - f) // 3) for f in (0, 1, 2, 0, 1, 2, 0)]):
        want = _scaled(codons_ref.codon_count(g, rows_all, regions), codons_ref.codon_count(g, rows_rem, regions), q)
        assert (len(want) + 1 <= LDS_CODONS) == (len(regions) == 3)
        eng.sample_codons(regions)
        summ, counts = eng.download_codons()
        assert (summ.rows, summ.n_codons, summ.n_regions) == (tallies["placed"], len(want), len(regions))
        assert np.array_equal(counts, want.astype(np.uint32)), np.argwhere(counts != want)[:5].tolist()
        assert mix == "all" or want.sum() > n

    # haplotypes
    regions = [(2052, 1), (2040, 12), (2030, 30), (2020, 64), (2011, 43), (2060, 3), (2000, 150)]
    one, two = haplotypes_ref.hap_count(g, rows_all, regions), haplotypes_ref.hap_count(g, rows_rem, regions)
    extra = {(r, h): cnt for r, cnt, h in two[2]}
    want = [(r, q * cnt + extra.get((r, h), 0), h) for r, cnt, h in one[2]]
    eng.sample_haplotypes(regions, 16)
    summ, cover, ref, entries = eng.download_haplotypes()
    assert (summ.rows, summ.n_regions, summ.dropped, summ.entries) == (tallies["placed"], len(regions), 0, len(want))
    assert np.array_equal(cover, _scaled(one[0], two[0], q)) and np.array_equal(ref, _scaled(one[1], two[1], q))
    assert entries == want, [x for x in zip(entries, want) if x[0] != x[1]][:3]
    assert mix == "all" or (len(want) >= 10 and cover[0] > n // 8 and cover[-1] == 0)
