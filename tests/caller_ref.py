"""The stages after the pileup restated a second time, in plain Python (tests only): get_baseline_noise (call.rs:799-967) and
call_variants (call.rs:969-1150), written from upstream's text -- not from oracle/bronko_oracle.c, bronko_amd/host/caller.cpp or
bk_caller.hip, which were all written from one reading of it.  Everything whose order or rounding matters is a Python float
(an IEEE double: +, -, *, / and math.sqrt are correctly rounded, one operation at a time) or a Python int; there is no numpy
reduction in here.  math.log and math.pow are the platform's, like every other restatement's.

Where upstream is not defined this module follows the project's definition and says so:
  * a sequence under 100 positions: upstream's `window_counts = vec![0.0; len*3]` (call.rs:813) is indexed (i % 100) * 3 + j and
    panics; the window here has 300 slots whatever the length, which is what upstream indexes for every length it survives;
  * all ten table entries stripped: upstream's `maxes[curr_max_idx]` (call.rs:957) panics at index 10; Noise.max is 0.0 here;
  * a sequence shorter than k under the end filter: `len - args.kmer` (call.rs:1015) underflows; no position is visited here;
  * a window of more than 300 values cannot exist (300 slots), so the Student-t table's range 3..300 is all there is.

Upstream's quirks are kept, each marked QUIRK below.
"""
import math
import os
import re

WINDOW = 100                    # call.rs:802
ALPHA = 0.001                   # call.rs:803 (folded into the tabulated quantile)
TABLE = WINDOW // 10            # call.rs:804
HALF = WINDOW // 2              # call.rs:824
NAN = float("nan")
INF = float("inf")

_TCRIT = None


def tcrit_table():
    """StudentsT(0, 1, n - 2).inverse_cdf(1 - 0.001 / n) for n = 3..300 (call.rs:924-925) from oracle/tcrit_table.inc: hex floats,
    one per line, C comments stripped.  tests/test_tcrit_independent.py checks the table itself."""
    global _TCRIT
    if _TCRIT is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "tcrit_table.inc")
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        _TCRIT = [float.fromhex(tok.strip()) for tok in text.split(",") if tok.strip()]
        assert len(_TCRIT) == 298
    return _TCRIT


def thompson_tau(n):
    """call.rs:922-929"""
    if n > 2:
        t_crit = tcrit_table()[n - 3] if n <= 300 else NAN
        return (t_crit * (float(n) - 1.0)) / (math.sqrt(float(n)) * math.sqrt(float(n) - 2.0 + t_crit * t_crit))
    return INF


def _sqrt(x):
    """f64::sqrt: NaN for a negative or NaN argument (math.sqrt raises)"""
    return math.sqrt(x) if x >= 0.0 else NAN


def baseline_noise(fwd4, rev4, evict_exact=False, trace=None):
    """get_baseline_noise (call.rs:799-967) of one sequence.  fwd4 / rev4: the depth counts in (position, base) order, 4 * len of
    them.  Returns three lists of len floats: Noise.max, Noise.mean, Noise.std per position.

    evict_exact: NOT upstream -- the eviction finds its entry by equality instead of `< 1e-12`.  The tests use it as a canary: inputs
    on which it gives the same answer say nothing about the 1e-12 rule.
    trace: a list that gets (values in the window, table entries stripped) for every position written."""
    fwd4 = [int(v) for v in fwd4]
    rev4 = [int(v) for v in rev4]
    length = len(fwd4) // 4
    out_max, out_mean, out_std = [0.0] * length, [0.0] * length, [0.0] * length
    window_counts = [0.0] * (WINDOW * 3)        # 300 slots: see the module's docstring
    in_max = [0] * (WINDOW * 3)
    maxes = [0.0] * TABLE
    n, s, s2 = 0, 0.0, 0.0
    for i in range(length + HALF):
        base_pos = (i % WINDOW) * 3
        if i < length:                                                      # call.rs:831-845
            counts = sorted((fwd4[i * 4 + b] + rev4[i * 4 + b] for b in range(4)), reverse=True)
            total_depth = sum(counts)
            freqs = [0.0] * 4 if total_depth == 0 else [float(c) / float(total_depth) for c in counts]
        else:
            freqs = [0.0] * 4
        for j in range(1, 4):                                               # call.rs:848
            idx = base_pos + (j - 1)
            old = window_counts[idx]
            if old > 0.0:                                                   # call.rs:854-870
                n -= 1
                s -= old
                s2 -= old * old
                if in_max[idx] == 1:
                    # QUIRK (call.rs:862): the FIRST entry within 1e-12 goes -- a larger neighbour of the leaving value if there is
                    # one, and an entry even when the leaving value itself never was in the table
                    pos = None
                    for q in range(TABLE):
                        if (maxes[q] == old) if evict_exact else (abs(maxes[q] - old) < 1e-12):
                            pos = q
                            break
                    if pos is not None:
                        for q in range(pos, TABLE - 1):
                            maxes[q] = maxes[q + 1]
                        maxes[TABLE - 1] = 0.0                              # QUIRK: the eleventh largest value does not move up
                    in_max[idx] = 0
            maf = freqs[j]                                                  # call.rs:873
            if maf > 0.0:
                n += 1
                s += maf
                s2 += maf * maf
                for q in range(TABLE - 1, -1, -1):                          # call.rs:880-889
                    if maf > maxes[q]:
                        if q + 1 < TABLE:
                            maxes[q + 1] = maxes[q]
                        maxes[q] = maf
                    else:
                        break
                in_max[idx] = 1                                             # QUIRK (call.rs:890): flagged whether it entered the table or not
            else:
                in_max[idx] = 0
            window_counts[idx] = maf                                        # call.rs:896
        if n != 0:                                                          # call.rs:901-907
            mu = s / float(n)
            var = (s2 / float(n)) - mu * mu
        else:
            mu, var = 0.0, 0.0
        cur, curr_n, curr_s, curr_s2, curr_mu, curr_var = 0, n, s, s2, mu, var
        while cur < TABLE and maxes[cur] != 0.0:                            # call.rs:917-950
            candidate = maxes[cur]
            std = _sqrt(curr_var)
            tau = thompson_tau(curr_n)
            if abs(candidate - curr_mu) > tau * std:                        # (inf * 0 = NaN: not an outlier)
                curr_s -= candidate
                curr_s2 -= candidate                                        # QUIRK (call.rs:936): the value, not its square
                curr_n -= 1
                if curr_n > 0:
                    curr_mu = curr_s / float(curr_n)
                    curr_var = (curr_s2 / float(curr_n)) - curr_mu * curr_mu
                else:
                    curr_mu, curr_var = 0.0, 0.0
                cur += 1
            else:
                break
        if i >= HALF:                                                       # call.rs:953-962
            w = i - HALF
            if w < length:
                out_max[w] = maxes[cur] if cur < TABLE else 0.0             # (index 10 panics upstream)
                out_mean[w] = curr_mu
                out_std[w] = _sqrt(curr_var)
                if trace is not None:
                    trace.append((n, cur))
    return out_max, out_mean, out_std


def call_variants(seqs, ref_codes, fwd, rev, fwd_nk, rev_nk, params, margins=None, noise=None):
    """call_variants (call.rs:969-1150) of one genome.  seqs: [(first cell, length)] of its sequences in metadata order (upstream
    walks a DashMap); ref_codes: nt_to_bits of every cell (non-ACGT is 0, lcb.rs:53); fwd, rev, fwd_nk, rev_nk: the four u64 arrays
    in (file, sequence, position, base) order; params: an object with the fields of CallArgs that call_variants reads (k, min_af,
    no_end_filter, no_strand_filter, no_strand_balance_filter, strand_balance_ratio, n_per_strand, strand_odds_max, min_depth,
    min_variant_depth, variant_multiplier).

    Returns (records, (n_major, n_minor, positions_covered, total_positions, total_coverage)); a record is a dict with the fields of
    VCFRecord, `seq_id` the index in seqs, in the order upstream pushes them.

    margins: a list that gets (seq_id, pos, alt, |sor - strand_odds_max| or None, |af - max(factor, y0) * noise| / af) for every
    (position, alternative) that reaches the test in question -- how far the decisions that go through ln() and pow() are from
    flipping.  noise: a list that gets each sequence's (max, mean, std)."""
    results = []
    num_minor, num_major = 0, 0
    positions_covered, total_positions, total_coverage = 0, 0, 0
    k = int(params.k)
    min_af, y0 = float(params.min_af), float(params.variant_multiplier)
    odds_max, balance_ratio = float(params.strand_odds_max), float(params.strand_balance_ratio)
    for seq_id, (cell0, length) in enumerate(seqs):
        c4 = cell0 * 4
        rows = [[int(v) for v in a[c4:c4 + 4 * length]] for a in (fwd, rev, fwd_nk, rev_nk)]
        nmax, nmean, nstd = baseline_noise(rows[0], rows[1])                # call.rs:1002
        if noise is not None:
            noise.append((nmax, nmean, nstd))
        start, end = 0, length
        if not params.no_end_filter:                                        # call.rs:1013-1016
            start, end = k, length - k                                      # (length < k: nothing, see the module's docstring)
        total_positions += length
        for i in range(start, end):
            row, row_rev = rows[0][i * 4:i * 4 + 4], rows[1][i * 4:i * 4 + 4]
            count, count_rev = rows[2][i * 4:i * 4 + 4], rows[3][i * 4:i * 4 + 4]
            ref_base = int(ref_codes[cell0 + i])
            row_total = [row[b] + row_rev[b] for b in range(4)]
            total_depth = sum(row_total)
            if total_depth == 0:
                continue
            positions_covered += 1
            total_coverage += total_depth
            for alt_base in range(4):
                if alt_base == ref_base or row_total[alt_base] == 0:
                    continue
                sor = odds_max + 1.0                                        # call.rs:1058
                sor_margin = None
                if not params.no_strand_filter:
                    a = float(row[ref_base]) + 1.0
                    b = float(row_rev[ref_base]) + 1.0
                    c = float(row[alt_base]) + 1.0
                    d = float(row_rev[alt_base]) + 1.0
                    ref_total = a + b + c + d
                    min_strand_percent = min(a + c, b + d) / ref_total
                    if (not params.no_strand_balance_filter) or min_strand_percent >= balance_ratio:
                        r = (a * d) / (b * c)                               # call.rs:1075-1079
                        ref_ratio = min(a, b) / max(a, b)
                        alt_ratio = min(c, d) / max(c, d)
                        sor = math.log(r + (1.0 / r)) + math.log(ref_ratio) - math.log(alt_ratio)
                        sor_margin = abs(sor - odds_max)
                        if sor > odds_max:
                            if margins is not None:
                                margins.append((seq_id, i + 1, alt_base, sor_margin, None))
                            continue
                        if count[alt_base] < params.n_per_strand and count_rev[alt_base] < params.n_per_strand:
                            if margins is not None:
                                margins.append((seq_id, i + 1, alt_base, sor_margin, None))
                            continue
                    else:
                        sor = -1.0                                          # call.rs:1094
                alt_count = row_total[alt_base]
                af = float(alt_count) / float(total_depth)                  # call.rs:1100
                factor = y0 + 0.5 * math.pow(0.03, 100.0 * af)              # call.rs:1102-1105
                bound = max(factor, y0) * nmax[i]
                if margins is not None:
                    margins.append((seq_id, i + 1, alt_base, sor_margin, abs(af - bound) / af))
                if af < min_af or af < bound:                               # call.rs:1107
                    continue
                if af >= 0.5:
                    num_major += 1
                else:
                    if total_depth < params.min_depth:                      # call.rs:1116
                        continue
                    if alt_count < params.min_variant_depth:                # call.rs:1119
                        continue
                    num_minor += 1
                results.append(dict(seq_id=seq_id, pos=i + 1, ref_base=ref_base, alt_base=alt_base, fwd_ref=row[ref_base],
                                    rev_ref=row_rev[ref_base], fwd_alt=row[alt_base], rev_alt=row_rev[alt_base], depth=total_depth,
                                    af=af, sor=sor))
    return results, (num_major, num_minor, positions_covered, total_positions, total_coverage)


def coverage(summary):
    """(breadth, depth) of call.rs:1144-1145 from call_variants' summary; depth is NaN when nothing is covered (0 / 0)"""
    _, _, covered, positions, cov = summary
    breadth = float(covered) / float(positions) if positions else NAN
    depth = float(cov) / float(covered) if covered else NAN
    return breadth, depth
