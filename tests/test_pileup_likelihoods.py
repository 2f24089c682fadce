"""--pileup-likelihoods, the parts that need no GPU: the table of terms, the rule (the new functions of
mapdamage_amd/csrc/mdx_pileup_key.h compiled for the host as the stand-alone program tests/pileup_gl_host.cpp, once more under
AddressSanitizer and UBSan, against the brute force of tests/gl_rule.py), the emitters of mapdamage_amd/pileup.py and the
command line's argument errors.  The device stage: tests/test_gpu_pileup_likelihoods.py."""

import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from tests import gl_rule as GR
from tests import pileup_rule as PR
from tests.test_pileup import (BASE, HAND_LENGTHS, HAND_LIBRARIES, HAND_RECORDS, HAND_SETTINGS, HAND_SITES, NAMES, batch_text, parse, random_records, rec,
                               site_offsets)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
M, I, D, N, S, H, P, EQ, X = range(9)
T = GR.TABLE


# ---------------------------------------------------------------------- the table
def test_table_rows():
    from mapdamage_amd import pileup
    table = pileup.likelihood_table()
    assert table.shape == (94, 3) and table.dtype == np.int64 and table.tolist() == GR.TABLE
    for q, row in ((0, (-23258160, -23258160, -23258160)), (1, (-23258160, -23258160, -23258160)), (2, (-16724251, -20786557, -26157849)),
                   (20, (-168617, -11741303, -95693591)), (30, (-16786, -11640269, -134324558)), (41, (-1333, -11629968, -176818622)),
                   (93, (0, -11629080, -377699653))):
        assert tuple(table[q].tolist()) == row, q
    assert all(table[q, 0] == table[q, 1] == table[q, 2] for q in (0, 1))          # e = 0.75: every genotype explains the base alike
    assert all(table[q + 1, 2] <= table[q, 2] for q in range(93)) and all(table[q + 1, 2] < table[q, 2] for q in range(1, 93))
    assert all(table[q + 1, 0] >= table[q, 0] for q in range(93)) and (table <= 0).all()
    assert all(table[q, 0] > table[q, 1] > table[q, 2] for q in range(2, 94))
    # fewer than 2^31 records are added, a record adds one term to a sum at the most: every sum stays inside an int64
    assert int(np.abs(table).max()) * 2**31 < 2**63


# ---------------------------------------------------------------------- the host program
@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("pileup_gl") / "pileup_gl_host"
    subprocess.check_call(["g++", *request.param, "-I", CSRC, os.path.join(ROOT, "tests", "pileup_gl_host.cpp"), "-o", str(exe)])

    def run(part, text, rows):
        out = subprocess.run([str(exe)], input=(part + "\n" + "\n".join(text) + "\n").encode(), capture_output=True, timeout=300)
        assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
        assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
        lines = out.stdout.decode().split("\n")
        assert lines[-2] == "OK" and len(lines) == rows + 2
        return lines[:rows]

    def sums(records, n_libraries, lengths, sites, k5=0, k3=0, min_qual=0, packed=False, noqual=30, single_strand=False, alleles=None):
        """-> (counters [sites][12], sums: a list of 24 per site, gl [sites][10], best, bases, the two counts)"""
        text = batch_text(records, n_libraries, lengths, k5, k3, min_qual, packed)
        text.append("%d %d %d %d" % (noqual, int(single_strand), len(sites), int(alleles is not None)))
        text.append(" ".join(str(int(x)) for x in site_offsets(sites, len(lengths))))
        text += ["%d" % p + ("" if alleles is None else " %d %d" % tuple(PR.BASES.index(a) for a in alleles[g])) for g, (_, p) in enumerate(sites)]
        text.append(" ".join(str(x) for row in GR.TABLE for x in row))
        lines = run("sums", text, len(sites) + 1)
        rows = [[int(x) for x in line.split()] for line in lines[:-1]]
        assert all(len(row) == 12 + 24 + 10 + 2 for row in rows)
        counts = dict(zip(("added", "without_qualities"), (int(x) for x in lines[-1].split())))
        return (np.array([row[:12] for row in rows], np.uint32).reshape(-1, 12), [row[12:36] for row in rows],
                np.array([row[36:46] for row in rows], np.int64).reshape(-1, 10), [row[46] for row in rows], [row[47] for row in rows], counts)

    def finish(rows, single_strand=False):
        """rows of (24 sums, 8 counters, ref, alt) -> [(the ten values, best, bases)]"""
        text = ["%d %d" % (len(rows), int(single_strand))] + [" ".join(map(str, list(s) + list(c) + [r, a])) for s, c, r, a in rows]
        out = [[int(x) for x in line.split()] for line in run("finish", text, len(rows))]
        return [(row[:10], row[10], row[11]) for row in out]

    class Host:
        pass
    h = Host()
    h.sums, h.finish = sums, finish
    return h


def against_the_rule(host, records, n_libraries, lengths, sites, k5=0, k3=0, min_qual=0, packed=False, noqual=30, single_strand=False, alleles=None):
    counters, sums, gl, best, bases, counts = host.sums(records, n_libraries, lengths, sites, k5, k3, min_qual, packed, noqual, single_strand, alleles)
    want_counters, _ = PR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual)
    want_sums, want_counts = GR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual, noqual)
    want_gl, want_best, want_bases = GR.all_likelihoods(want_sums, want_counters, alleles, single_strand)
    assert (counters == want_counters).all()
    assert sums == want_sums, [(sites[g], sums[g], want_sums[g]) for g in range(len(sites)) if sums[g] != want_sums[g]][:3]
    assert (gl == want_gl).all() and best == want_best and bases == want_bases and counts == want_counts
    assert (gl <= 0).all() and all(gl[g, best[g]] == 0 for g in range(len(sites)))
    return want_sums, want_gl, want_best, want_bases, want_counts


# ---------------------------------------------------------------------- the rule
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
def test_hand_written_records(host, packed):
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(HAND_SITES))]
    for n, (k5, k3, q) in enumerate(HAND_SETTINGS):
        _, _, _, bases, counts = against_the_rule(host, HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, k5, k3, q, packed, noqual=(30, 7)[n % 2],
                                                  single_strand=bool(n % 2), alleles=alleles if n % 3 else None)
        counters, _ = PR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, k5, k3, q)
        assert counts["added"] == int(counters[:, :8].sum())                        # a pair adds exactly where it adds to a base counter
    assert counts["added"] == 0                                                     # (windows longer than every read: every base Masked)


def test_the_yardstick_by_hand():
    """Sites of the hand-written table worked out from the table's rows, so that the brute force is itself held to something."""
    counters, _ = PR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, 0, 0, 20)
    sums, counts = GR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, 0, 0, 20, noqual=7)
    at = lambda t, p: HAND_SITES.index((t, p))
    row = lambda cls, q: [T[q][k] if c == cls else 0 for c in range(8) for k in range(3)]
    add = lambda *rows: [sum(x) for x in zip(*rows)]
    assert sums[at(0, 9)] == [0] * 24
    assert sums[at(0, 39)] == row(3, 30)                                            # T+ at quality 30
    assert sums[at(0, 380)] == row(0, 7)                                            # A+ of the record without qualities, at the noqual quality
    assert sums[at(0, 395)] == row(0, 20)                                           # A+ at exactly Q = 20; the reverse record's 19 is LowQual
    assert sums[at(0, 397)] == add(row(2, 20), row(6, 21)) and sums[at(0, 398)] == row(4, 93)
    assert sums[at(0, 10)] == add(row(2, 30), row(7, 30), row(1, 30))               # G+, T-, and the paired record's C+
    # one base: T+ at 30.  TT is best; a genotype with one T loses HOM - HET, one without loses HOM - NO
    gl, best, bases = GR.likelihoods(sums[at(0, 39)], counters[at(0, 39)])
    hom, het, no = T[30]
    assert (best, bases) == (9, 1) and gl == [no - hom, no - hom, no - hom, het - hom, no - hom, no - hom, het - hom, no - hom, het - hom, 0]
    # two different bases: G+ at 20, G- at 21 -> the same base on both strands: GG
    gl, best, bases = GR.likelihoods(sums[at(0, 397)], counters[at(0, 397)])
    assert (best, bases) == (7, 2) and gl[2] == T[20][1] + T[21][1] - T[20][0] - T[21][0] and gl[0] == T[20][2] + T[21][2] - T[20][0] - T[21][0]
    # G+, T-, C+ at 30: the three heterozygotes of two of them tie in front, the first in the order is CG
    gl, best, bases = GR.likelihoods(sums[at(0, 10)], counters[at(0, 10)])
    assert bases == 3 and gl[5] == gl[6] == gl[8] == 0 and best == 5 and gl[4] == gl[7] == gl[9] == hom + 2 * no - (2 * het + no)
    assert counts["without_qualities"] == 2                                         # the record without qualities lies over the sites 380 and 389


def test_sites_by_hand(host):
    """The ten values from the table's rows: one base, two different bases, the same base on both strands, and ties."""
    row = lambda *pairs: [sum(T[q][k] for c, q in pairs if c == cls) for cls in range(8) for k in range(3)]
    count = lambda *pairs: [sum(1 for c, _ in pairs if c == cls) for cls in range(8)]
    hom, het, no = T[30]
    cases = [
        # one A+ at 30
        ([(0, 30)], [0, het - hom, het - hom, het - hom, no - hom, no - hom, no - hom, no - hom, no - hom, no - hom], 0, 1),
        # A+ at 30 and C- at 30: AC is best
        ([(0, 30), (5, 30)], [hom + no - 2 * het, 0, het + no - 2 * het, het + no - 2 * het, hom + no - 2 * het, het + no - 2 * het, het + no - 2 * het,
                              2 * no - 2 * het, 2 * no - 2 * het, 2 * no - 2 * het], 1, 2),
        # G+ at 20 and G- at 41
        ([(2, 20), (6, 41)], None, 7, 2),
        # quality 0 and 1: every genotype alike, the first is the best
        ([(3, 0), (1, 1)], [0] * 10, 0, 2),
        # nothing
        ([], [0] * 10, 0, 0),
        # A+ and T+ at 30: AT alone in front; A+ C+ G+ T+: the six heterozygotes tie, AC first
        ([(0, 30), (3, 30)], None, 3, 2),
        ([(0, 30), (1, 30), (2, 30), (3, 30)], [hom + 3 * no - (2 * het + 2 * no), 0, 0, 0, hom + 3 * no - (2 * het + 2 * no), 0, 0,
                                                hom + 3 * no - (2 * het + 2 * no), 0, hom + 3 * no - (2 * het + 2 * no)], 1, 4),
        # two C- against one T+ of a better quality
        ([(5, 20), (5, 20), (3, 41)], None, None, 3),
    ]
    got = host.finish([(row(*pairs), count(*pairs), -1, -1) for pairs, _, _, _ in cases])
    for (pairs, gl, best, bases), (got_gl, got_best, got_bases) in zip(cases, got):
        want = GR.likelihoods(row(*pairs), count(*pairs) + [0] * 4)
        assert (got_gl, got_best, got_bases) == want, pairs
        assert got_bases == bases and (best is None or got_best == best) and (gl is None or got_gl == gl), pairs
    g20, g41 = T[20], T[41]
    assert got[2][0][7] == 0 and got[2][0][0] == g20[2] + g41[2] - g20[0] - g41[0] and got[2][0][2] == g20[1] + g41[1] - g20[0] - g41[0]
    # 2 x C at 20 against T at 41: CT = 2 het20 + het41 beats CC = 2 hom20 + no41 and TT = 2 no20 + hom41
    assert got[7][1] == 6 and got[7][0][4] == 2 * g20[0] + g41[2] - (2 * g20[1] + g41[1])
    # sums as large as the limit allows: 2^31 - 1 bases at quality 93 on one strand and base
    big = 2**31 - 1
    s = [0] * 24
    s[3 * 6:3 * 6 + 3] = [big * x for x in T[93]]
    (gl, best, bases), = host.finish([(s, [0, 0, 0, 0, 0, 0, big, 0], -1, -1)])
    assert (gl, best, bases) == GR.likelihoods(s, [0, 0, 0, 0, 0, 0, big, 0, 0, 0, 0, 0]) and best == 7 and gl[0] == big * (T[93][2] - T[93][0]) and bases == big


def test_single_strand_mode(host):
    """C/T: the - strand alone; G/A: the + strand alone; a transversion: both.  All four bases stay in the sums, whatever the
    alleles."""
    pairs = [(0, 30), (1, 20), (1, 20), (3, 41), (4, 30), (5, 41), (6, 2), (6, 20), (7, 93)]
    row = [sum(T[q][k] for c, q in pairs if c == cls) for cls in range(8) for k in range(3)]
    count = [sum(1 for c, _ in pairs if c == cls) for cls in range(8)]
    sites = [(row, count, r, a) for r, a in ((1, 3), (3, 1), (2, 0), (0, 2), (0, 1), (2, 3), (-1, -1))]
    on, off = host.finish(sites, True), host.finish(sites, False)
    letters = lambda r, a: None if r < 0 else (PR.BASES[r], PR.BASES[a])
    for (s, c, r, a), got_on, got_off in zip(sites, on, off):
        assert got_on == GR.likelihoods(s, c + [0] * 4, letters(r, a), True) and got_off == GR.likelihoods(s, c + [0] * 4, letters(r, a), False)
    assert [x[2] for x in on] == [5, 5, 4, 4, 9, 9, 9] and [x[2] for x in off] == [9] * 7
    assert on[0] == on[1] != off[0] and on[2] == on[3] != on[0] and on[4] == on[5] == on[6] == off[0]
    # the - strand alone is what a site holds whose + strand is empty
    minus_only = GR.likelihoods([0] * 12 + row[12:], [0] * 4 + count[4:] + [0] * 4)
    assert on[0] == minus_only
    # ... through the records, too
    records = [rec(0, 0, 0, 10, [(M, 8)], "CCTTGGAA"), rec(0x10, 0, 0, 10, [(M, 8)], "TTCCAAGG", [20] * 8), rec(0x10, 1, 0, 12, [(M, 4)], "TTGA", None)]
    sites = [(0, p) for p in range(9, 19)]
    alleles = ["CT", "CT", "TC", "CT", "TC", "GA", "AG", "AG", "AC", "GT"]
    _, gl, _, bases, _ = against_the_rule(host, records, 3, [100], sites, single_strand=True, alleles=alleles, noqual=12)
    assert bases == [0, 1, 1, 2, 2, 1, 1, 1, 2, 0]


def test_records_without_qualities(host):
    """No quality column at all, a first byte of 0xFF, and both beside records with qualities: the noqual quality, counted apart;
    --pileup-min-basequal does not touch them."""
    sites = [(0, p) for p in range(0, 60, 3)]
    none = [rec(0, 0, 0, 5, [(M, 30)], qual=None), rec(0x10, 1, 0, 20, [(M, 10), (D, 2), (M, 10)], qual=None)]
    for noqual in (1, 30, 93):
        sums, _, _, _, counts = against_the_rule(host, none, 2, [100], sites, min_qual=40, noqual=noqual)
        assert counts["added"] == counts["without_qualities"] == 16
        assert all(x % T[noqual][k % 3] == 0 for row in sums for k, x in enumerate(row) if x)
    mixed = none + [rec(0, 0, 0, 0, [(M, 50)], qual=[0xFF] + [10] * 49), rec(0, 1, 0, 0, [(M, 50)], qual=[10] + [0xFF] * 49), rec(0, 0, 0, 30, [(M, 9)], "ACGTNACGT")]
    for packed in (False, True):
        _, _, _, _, counts = against_the_rule(host, mixed, 2, [100], sites, min_qual=5, noqual=9, packed=packed)
        assert counts["without_qualities"] == 16 + 17 and counts["added"] == 16 + 17 + 17 + 3           # (the N at 34 lies over no site)


def test_quality_bytes_at_the_table_s_ends(host):
    """0, 1 and 2; 93, and 94 and 254 that are taken at 93; 255 inside a record with qualities."""
    quals = [0, 1, 2, 93, 94, 254, 255, 40, 3]
    records = [rec(0, 0, 0, 10, [(M, 9)], "ACGTACGTA", [30] + quals[1:]), rec(0x10, 0, 0, 10, [(M, 9)], "A" * 9, quals)]
    sites = [(0, p) for p in range(10, 19)]
    sums, gl, best, bases, counts = against_the_rule(host, records, 1, [50], sites)
    assert counts == dict(added=18, without_qualities=0)
    for k, q in enumerate(quals):
        assert sums[k][12:15] == T[min(q, 93)], q
    assert sums[4][12:15] == sums[5][12:15] == sums[6][12:15] == T[93] == sums[3][12:15]
    assert sums[1][3:6] == sums[1][12:15] == T[0]


@pytest.mark.parametrize("seed,packed", [(1, False), (2, True)])
def test_rule_on_random_records(host, seed, packed):
    lengths = [400, 1, 0, 150]
    records = random_records(seed, 2500, lengths) + [rec(0, 0, 1, 0, [(S, 3), (M, 1)]), rec(0x10, 2, 1, 0, [(EQ, 1), (I, 2)])]
    rng = np.random.default_rng(seed)
    sites = sorted({(0, int(p)) for p in rng.choice(400, 150, replace=False)} | {(1, 0)} | {(3, p) for p in range(150)})
    alleles = [tuple(PR.BASES[int(b)] for b in rng.choice(4, 2, replace=False)) for _ in sites]
    k5, k3, q = [(2, 3, 15), (5, 0, 30)][seed - 1]
    _, gl, best, bases, counts = against_the_rule(host, records, 3, lengths, sites, k5, k3, q, packed, noqual=25, single_strand=True, alleles=alleles)
    assert counts["added"] > 500 and counts["without_qualities"] > 50 and len(set(best)) >= 8 and 0 in bases and max(bases) >= 5


def test_ties_take_the_first_genotype(host):
    """Equal values at the top: the first in AA AC AG AT CC CG CT GG GT TT."""
    row = lambda *pairs: [sum(T[q][k] for c, q in pairs if c == cls) for cls in range(8) for k in range(3)]
    count = lambda *pairs: [sum(1 for c, _ in pairs if c == cls) for cls in range(8)]
    cases = [([(3, 1)], 0), ([(2, 30), (7, 30)], 8), ([(1, 30), (2, 30), (3, 30)], 5), ([(0, 0), (1, 0), (6, 1)], 0), ([(2, 30), (3, 30), (6, 1)], 8),
             ([(1, 30), (4, 30), (7, 30)], 1)]
    got = host.finish([(row(*pairs), count(*pairs), -1, -1) for pairs, _ in cases])
    for (pairs, first), (gl, best, bases) in zip(cases, got):
        assert best == first and gl[first] == 0 and all(v < 0 for v in gl[:first]) and (gl, best, bases) == GR.likelihoods(row(*pairs), count(*pairs) + [0] * 4), pairs
    assert sum(1 for v in got[2][0] if v == 0) == 3 and sum(1 for v in got[5][0] if v == 0) == 3


# ---------------------------------------------------------------------- the emitters
def some_values():
    sites = parse("chrM\t3\tC\tT\trs2\nchr1\t10\tA\tG\trs1\nscaf/1:a\t7\tG\tC\nchr1\t11\tT\tA\trs4\n")
    pairs = [[(0, 30), (2, 20), (6, 41)], [], [(1, 2), (5, 93), (7, 11)], [(2, 40)] * 300 + [(5, 40)] * 280]
    sums = [[sum(T[q][k] for c, q in site if c == cls) for cls in range(8) for k in range(3)] for site in pairs]
    counters = [[sum(1 for c, _ in site if c == cls) for cls in range(8)] + [0] * 4 for site in pairs]
    site_list = list(zip(sites.tid.tolist(), sites.pos.tolist()))
    alleles = ["AG", "TA", "CT", "GC"]
    gl, best, bases = GR.all_likelihoods(sums, counters)
    return sites, site_list, alleles, gl, np.array(best, np.uint8), np.array(bases, np.uint32)


def test_emitters(tmp_path, monkeypatch):
    from mapdamage_amd import pileup
    sites, site_list, alleles, gl, best, bases = some_values()
    text = b"".join(pileup.likelihoods_chunks(NAMES, sites, gl, best, bases)).decode()
    want = GR.likelihoods_text(NAMES, site_list, sites.ids, alleles, gl, best, bases)
    assert GR.same_text(text, want, GR.LIKELIHOOD_FLOATS)
    lines = text.split("\n")
    assert lines[0] == "Sequence\tPosition\tId\tRef\tAlt\tBases\tAA\tAC\tAG\tAT\tCC\tCG\tCT\tGG\tGT\tTT\tBest"
    assert lines[2] == "chr1\t11\trs4\tT\tA\t0" + "\t0.000000" * 10 + "\t." and lines[1].startswith("chr1\t10\trs1\tA\tG\t3\t") and lines[1].endswith("\tAG")
    # a value by hand: one unit of the last place is 2^-24 / ln 10
    fields = lines[1].split("\t")
    assert abs(float(fields[6]) - int(gl[0, 0]) / 2**24 / math.log(10)) <= 5.01e-7 and fields[8] == "0.000000" and float(fields[6]) < -1
    assert b"".join(pileup.likelihoods_chunks(NAMES, sites, gl, best, bases, chunk=3)).decode() == text
    plain = parse("chrM\t3\nchr1\t10\nscaf/1:a\t7\nchr1\t11\n")
    assert GR.same_text(b"".join(pileup.likelihoods_chunks(NAMES, plain, gl, best, bases)).decode(), GR.likelihoods_text(NAMES, site_list, None, None, gl, best, bases),
                        GR.LIKELIHOOD_FLOATS)
    pileup.write_likelihoods(tmp_path / "pileup_likelihoods.tsv", NAMES, sites, gl, best, bases)
    assert (tmp_path / "pileup_likelihoods.tsv").read_text() == text and os.listdir(tmp_path) == ["pileup_likelihoods.tsv"]
    # the summary and the log line
    counts = dict(added=586, without_qualities=7)
    values = dict(path="panel.txt", min_basequal=20, mask_ends=(2, 3), single_strand=True, noqual_quality=25)
    assert pileup.likelihoods_summary_text(values, bases, counts) == GR.summary_text("panel.txt", 20, 2, 3, True, 25, bases.tolist(), counts) == (
        "SitesFile\tMinBaseQual\tMaskEnds\tSingleStrandMode\tNoQualQuality\tSites\tSitesWithBases\tBaseObservations\tWithoutQualities\n"
        "panel.txt\t20\t2,3\t1\t25\t4\t3\t586\t7\n")
    assert pileup.likelihoods_log_line(values, bases, counts) == GR.log_line(25, bases.tolist(), counts) == (
        "Pileup likelihoods: 4 sites, 3 with bases, 586 base observations (7 from records without qualities, taken at 25)")
    # a failure on the way removes the temporary file and leaves an earlier file alone
    def broken(*args, **kwargs):
        yield b"Sequence\n"
        raise OSError("disk full")
    monkeypatch.setattr(pileup, "likelihoods_chunks", broken)
    with pytest.raises(OSError):
        pileup.write_likelihoods(tmp_path / "pileup_likelihoods.tsv", NAMES, sites, gl, best, bases)
    assert os.listdir(tmp_path) == ["pileup_likelihoods.tsv"] and (tmp_path / "pileup_likelihoods.tsv").read_text() == text


def test_beagle(tmp_path, monkeypatch):
    from mapdamage_amd import pileup
    sites, site_list, alleles, gl, best, bases = some_values()
    text = b"".join(pileup.beagle_chunks(NAMES, sites, gl, bases)).decode()
    assert GR.same_text(text, GR.beagle_text(NAMES, site_list, alleles, gl, bases), GR.BEAGLE_FLOATS)
    lines = text.split("\n")
    assert lines[0] == "marker\tallele1\tallele2\tInd0\tInd0\tInd0" and lines[2] == "chr1_11\t3\t0\t0.333333\t0.333333\t0.333333"
    assert lines[1].startswith("chr1_10\t0\t2\t") and lines[3].startswith("chrM_3\t1\t3\t") and lines[4].startswith("scaf/1:a_7\t2\t1\t")
    for line in lines[1:-1]:
        three = [float(x) for x in line.split("\t")[3:]]
        assert abs(sum(three) - 1) <= 2e-6 and all(0 <= x <= 1 for x in three)
    # site 0: ref A, alt G -> AA, AG, GG by hand
    three = [math.exp(int(gl[0, g]) / 2**24) for g in (0, 2, 7)]
    assert all(abs(float(x) - y / sum(three)) <= 5.01e-7 for x, y in zip(lines[1].split("\t")[3:], three))
    assert b"".join(pileup.beagle_chunks(NAMES, sites, gl, bases, chunk=1)).decode() == text
    # a deep site whose bases are neither allele (580 of T and A under G/C): the three genotypes explain them alike, a third
    # each, where exp() of any of them alone is 0
    deep = [sum(T[40][k] for _ in range(n)) if n else 0 for n in (0, 0, 0, 300, 280, 0, 0, 0) for k in range(3)]
    deep_gl, _, deep_bases = GR.likelihoods(deep, [0, 0, 0, 300, 280, 0, 0, 0, 0, 0, 0, 0])
    assert math.exp(deep_gl[4] / 2**24) == 0.0 and deep_gl[4] == deep_gl[5] == deep_gl[7]
    one = parse("chr1\t7\tG\tC\n")
    assert b"".join(pileup.beagle_chunks(NAMES, one, np.array([deep_gl], np.int64), np.array([deep_bases], np.uint32))).decode().split("\n")[1] == (
        "chr1_7\t2\t1\t0.333333\t0.333333\t0.333333")
    assert [pileup.genotype_index(a, b) for a in range(4) for b in range(a, 4)] == list(range(10)) and pileup.genotype_index(3, 1) == 6
    # plain and gzip, the latter the same bytes whenever it is written
    pileup.write_beagle(tmp_path / "out.beagle", NAMES, sites, gl, bases)
    pileup.write_beagle(tmp_path / "out.beagle.gz", NAMES, sites, gl, bases)
    packed = (tmp_path / "out.beagle.gz").read_bytes()
    assert (tmp_path / "out.beagle").read_text() == text == gzip.decompress(packed).decode()
    assert packed[:4] == b"\x1f\x8b\x08\x00" and packed[4:8] == b"\0\0\0\0"        # no name, a zero mtime
    pileup.write_beagle(tmp_path / "again.gz", NAMES, sites, gl, bases)
    assert (tmp_path / "again.gz").read_bytes() == packed and sorted(os.listdir(tmp_path)) == ["again.gz", "out.beagle", "out.beagle.gz"]
    def broken(*args, **kwargs):
        yield b"marker\n"
        raise OSError("disk full")
    monkeypatch.setattr(pileup, "beagle_chunks", broken)
    for name in ("out.beagle", "out.beagle.gz", "new.gz"):
        with pytest.raises(OSError):
            pileup.write_beagle(tmp_path / name, NAMES, sites, gl, bases)
    assert sorted(os.listdir(tmp_path)) == ["again.gz", "out.beagle", "out.beagle.gz"] and (tmp_path / "out.beagle.gz").read_bytes() == packed


# ---------------------------------------------------------------------- the command line
@pytest.fixture()
def site_files(tmp_path):
    (tmp_path / "plain.txt").write_text("# sites\nchr1\t5\nchr1\t9\n")
    (tmp_path / "alleles.txt").write_text("chr1\t5\tA\tG\trs1\n")
    (tmp_path / "in.bam").write_bytes(b"")
    return tmp_path


@pytest.mark.parametrize("extra,words", [
    (["--pileup-sites", "{alleles}", "--pileup-noqual-quality", "20"], "--pileup-noqual-quality needs --pileup-likelihoods"),
    (["--pileup-sites", "{alleles}", "--pileup-beagle", "{dir}/x.beagle"], "--pileup-beagle needs --pileup-likelihoods"),
    (["--pileup-noqual-quality", "20", "--pileup-beagle", "{dir}/x.beagle"], "--pileup-noqual-quality / --pileup-beagle need --pileup-likelihoods"),
    (["--pileup-likelihoods"], "--pileup-likelihoods needs --pileup-sites"),
    (["--pileup-likelihoods", "--pileup-noqual-quality", "20"], "--pileup-likelihoods needs --pileup-sites"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "-Q", "20"], "--pileup-likelihoods cannot be combined with -Q 20"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-min-basequal", "20", "-Q", "20"], "--pileup-likelihoods cannot be combined with -Q 20"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-beagle", "{dir}/x.beagle"], "--pileup-beagle needs Ref and Alt on every site"),
    (["--pileup-sites", "{alleles}", "--pileup-likelihoods", "--pileup-beagle", "{dir}/none/x.beagle"], "x.beagle: its directory does not exist"),
    (["-i", "{dir}/in.bam", "--pileup-sites", "{alleles}", "--pileup-likelihoods", "--pileup-beagle", "{dir}/in.bam"], "in.bam is the input file"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-noqual-quality", "0"], "--pileup-noqual-quality 0: a quality of 1..93"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-noqual-quality", "94"], "--pileup-noqual-quality 94: a quality of 1..93"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-noqual-quality", "-5"], "--pileup-noqual-quality -5: a quality of 1..93"),
    # every restriction of --pileup-sites stands
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--host-decode"], "not with --host-decode"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--gpus", "2"], "--pileup-sites cannot be combined with --gpus 2"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "-n", "5000"], "--pileup-sites cannot be combined with -n 5000"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--rescale-only"], "--pileup-sites belongs to the tabulation pass"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-single-strand-mode"], "--pileup-single-strand-mode needs Ref and Alt on every site"),
])
def test_argument_errors(capsys, site_files, extra, words):
    from mapdamage_amd.main import parse_args
    files = dict(plain=site_files / "plain.txt", alleles=site_files / "alleles.txt", dir=site_files)
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + [e.format(**files) for e in extra])
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_arguments_that_pass(site_files):
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "plain.txt"), "--pileup-likelihoods"])
    assert o.pileup_likelihoods and o.pileup_noqual_quality == 30 and o.pileup_beagle is None
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "alleles.txt"), "--pileup-likelihoods", "--pileup-noqual-quality", "93", "--pileup-beagle",
                           str(site_files / "x.beagle.gz"), "--pileup-min-basequal", "20", "--pileup-mask-ends", "2,1", "--pileup-single-strand-mode",
                           "--remove-duplicates", "--depth", "--by-pmd-score"])
    assert o.pileup_noqual_quality == 93 and o.pileup_beagle == str(site_files / "x.beagle.gz") and o.pileup_min_basequal == 20
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "plain.txt")])
    assert not o.pileup_likelihoods and o.pileup_noqual_quality is None and o.pileup_beagle is None
    o = parse_args(BASE)
    assert not o.pileup_likelihoods and o.pileup_noqual_quality is None
