"""--pileup-damage-profile, the parts that need no GPU: the profile's parser, the table of terms, the rule (the new functions of
mapdamage_amd/csrc/mdx_pileup_key.h compiled for the host as the stand-alone program tests/pileup_gld_host.cpp, once more under
AddressSanitizer and UBSan, against the brute force of tests/gld_rule.py), the emitters of mapdamage_amd/pileup.py and the command
line's argument errors.  The device stage: tests/test_gpu_pileup_damage_likelihoods.py."""

import math
import os
import subprocess

import numpy as np
import pytest

from tests import gl_rule as GR
from tests import gld_rule as DR
from tests import pileup_rule as PR
from tests.test_pileup import BASE, HAND_LENGTHS, HAND_LIBRARIES, HAND_RECORDS, HAND_SETTINGS, HAND_SITES, batch_text, random_records, rec, site_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
M, I, D, N, S, H, P, EQ, X = range(9)
A, C, G, T = range(4)
AA, AC, AG, AT, CC, CG, CT, GG, GT, TT = range(10)


def rows_of(rates_, bases=1000):
    """[(substitutions, bases)] whose quotients are about ``rates_``."""
    return [(round(r * bases), bases) for r in rates_]


# a profile of 30 positions: strong damage at the ends that falls off, different at either end; the tail pools 6 .. 30 (K = 5)
ROWS5 = rows_of([0.31, 0.17, 0.09, 0.06, 0.04, 0.03] + [0.012] * 24, 997)
ROWS3 = rows_of([0.27, 0.12, 0.08, 0.05, 0.035, 0.02] + [0.009] * 24, 1013)
TEXT = DR.misincorporation_text(ROWS5, ROWS3, libraries=(("s", "a"), ("s", "b")))
D5_K5, D3_K5 = DR.profile(TEXT, 5)
D5_K20, D3_K20 = DR.profile(TEXT, 20)
ZERO5, ZERO3 = DR.profile(DR.misincorporation_text([(0, 50)] * 8, [(0, 60)] * 8), 3)


# ---------------------------------------------------------------------- the profile
def test_profile_summed_by_hand():
    from mapdamage_amd import pileup
    text = ("Sample\tLibrary\tEnd\tStd\tPos\tA\tC\tG\tT\tTotal\tG>A\tC>T\tA>G\n"
            "s\ta\t5p\t+\t1\t9\t100\t50\t9\t168\t5\t30\t0\n"
            "s\ta\t5p\t-\t1\t9\t60\t50\t9\t128\t5\t10\t0\n"
            "s\tb\t5p\t+\t1\t9\t40\t50\t9\t108\t5\t10\t0\n"
            "s\tb\t5p\t-\t1\t9\t0\t50\t9\t68\t5\t0\t0\n"
            "s\ta\t5p\t+\t2\t9\t80\t50\t9\t148\t50\t8\t0\n"
            "s\tb\t5p\t-\t2\t9\t20\t50\t9\t88\t50\t2\t0\n"
            "s\ta\t5p\t+\t3\t9\t30\t50\t9\t98\t1\t3\t0\n"
            "s\tb\t5p\t+\t4\t9\t70\t50\t9\t138\t1\t1\t0\n"
            "s\ta\t3p\t+\t1\t9\t77\t40\t9\t135\t12\t70\t0\n"
            "s\tb\t3p\t-\t1\t9\t77\t10\t9\t105\t3\t70\t0\n"
            "s\ta\t3p\t-\t2\t9\t77\t25\t9\t120\t2\t1\t0\n"
            "s\ta\t3p\t-\t3\t9\t77\t20\t9\t115\t1\t1\t0\n"
            "s\tb\t3p\t-\t4\t9\t77\t30\t9\t125\t2\t1\t0\n")
    p = pileup.parse_damage_profile(text.split("\n"), 2, "x.txt")
    assert (p.positions, p.largest, p.path) == (2, 4, "x.txt")
    assert p.ends[0] == [(50, 200, 0.25), (10, 100, 0.1), (4, 100, 0.04)]              # the tail: positions 3 and 4 pooled
    assert p.ends[1] == [(15, 50, 0.3), (2, 25, 0.08), (3, 50, 0.06)]
    assert (p.ends[0], p.ends[1]) == DR.profile(text, 2)
    p = pileup.parse_damage_profile(text.split("\n"), 3)
    assert p.ends[0] == [(50, 200, 0.25), (10, 100, 0.1), (3, 30, 0.1), (1, 70, 1 / 70)] and (p.ends[0], p.ends[1]) == DR.profile(text, 3)


def test_profile_of_a_written_table_and_of_a_reference_style_file(tmp_path):
    from mapdamage_amd import pileup
    for k in (1, 5, 20, 29):
        p = pileup.parse_damage_profile(TEXT.split("\n"), k)
        assert (p.ends[0], p.ends[1]) == DR.profile(TEXT, k) and p.largest == 30 and len(p.ends[0]) == k + 1
        assert [row[:2] for row in p.ends[0][:k]] == ROWS5[:k] and p.ends[1][k][:2] == (sum(s for s, _ in ROWS3[k:]), sum(b for _, b in ROWS3[k:]))
    # mapDamage's own: comment lines, an empty line, a Chr column and no Sample / Library; \r\n line ends
    style = DR.misincorporation_text(ROWS5, ROWS3, comments=True)
    assert style.startswith("# table produced by mapDamage\n") and "\n\nChr\tEnd\tStd\tPos" in style
    for text in (style, style.replace("\n", "\r\n")):
        (tmp_path / "misincorporation.txt").write_bytes(text.encode())
        p = pileup.read_damage_profile(tmp_path / "misincorporation.txt", 5)
        assert (p.ends[0], p.ends[1]) == (D5_K5, D3_K5) and p.path == str(tmp_path / "misincorporation.txt")


def test_profile_positions_without_data():
    from mapdamage_amd import pileup
    rows5 = [(30, 100), (0, 0), (0, 0), (5, 100), (0, 0), (2, 100), (1, 100)]
    rows3 = [(20, 100), (10, 100), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)]
    text = DR.misincorporation_text(rows5, rows3)
    p = pileup.parse_damage_profile(text.split("\n"), 5)
    assert p.ends[0] == [(30, 100, 0.3), (0, 0, 0.3), (0, 0, 0.3), (5, 100, 0.05), (0, 0, 0.05), (3, 200, 0.015)]
    assert p.ends[1] == [(20, 100, 0.2), (10, 100, 0.1)] + [(0, 0, 0.1)] * 4           # a tail without data: the rate in front of it
    assert (p.ends[0], p.ends[1]) == DR.profile(text, 5)
    for rows, end, base in (([(0, 0)] + rows5[1:], "5p", "C"), ):
        with pytest.raises(pileup.ProfileError) as error:
            pileup.parse_damage_profile(DR.misincorporation_text(rows, rows3).split("\n"), 5, "t.txt")
        assert "t.txt" in str(error.value) and "position 1" in str(error.value) and end in str(error.value)
    with pytest.raises(pileup.ProfileError) as error:
        pileup.parse_damage_profile(DR.misincorporation_text(rows5, [(0, 0)] + rows3[1:]).split("\n"), 5, "t.txt")
    assert "position 1 of the 3p rows" in str(error.value)
    with pytest.raises(ValueError):
        DR.profile(DR.misincorporation_text([(0, 0)] + rows5[1:], rows3), 5)


HEAD = "End\tStd\tPos\tA\tC\tG\tT\tTotal\tG>A\tC>T"
GOOD = [HEAD, "5p\t+\t1\t1\t10\t10\t1\t22\t1\t3", "5p\t+\t2\t1\t10\t10\t1\t22\t1\t1", "3p\t+\t1\t1\t10\t10\t1\t22\t2\t1", "3p\t+\t2\t1\t10\t10\t1\t22\t1\t1"]


@pytest.mark.parametrize("lines,k,words", [
    ([HEAD.replace("\tC>T", "")] + GOOD[1:], 1, "line 1: the header lacks the column C>T"),
    ([HEAD.replace("End", "end").replace("G>A", "G>a")] + GOOD[1:], 1, "the header lacks the columns End, G>A"),
    (["# only a comment", ""], 1, "holds no header line"),
    (GOOD[:2] + ["5p\t+\tx\t1\t10\t10\t1\t22\t1\t1"] + GOOD[3:], 1, "line 3: Pos is 'x', not a non-negative integer"),
    (GOOD[:2] + ["5p\t+\t-2\t1\t10\t10\t1\t22\t1\t1"] + GOOD[3:], 1, "line 3: Pos is '-2', not a non-negative integer"),
    (GOOD[:2] + ["5p\t+\t0\t1\t10\t10\t1\t22\t1\t1"] + GOOD[3:], 1, "line 3: Pos is 0"),
    (GOOD[:2] + ["5p\t+\t2\t1\t1.5\t10\t1\t22\t1\t1"] + GOOD[3:], 1, "line 3: C is '1.5', not a non-negative integer"),
    (GOOD[:3] + ["3p\t+\t1\t1\t10\t10\t1\t22\t\t1"] + GOOD[4:], 1, "line 4: G>A is '', not a non-negative integer"),
    (["# c"] + GOOD[:3] + ["3p\t+\t1\t1\t10\t10\t1"] + GOOD[4:], 1, "line 5: 7 fields"),
    (GOOD[:2] + ["5'\t+\t2\t1\t10\t10\t1\t22\t1\t1"] + GOOD[3:], 1, "line 3: End is \"5'\", neither 5p nor 3p"),
    (GOOD[:2] + ["5p\t+\t2\t1\t10\t10\t1\t22\t1\t11"] + GOOD[3:], 1, "line 3: C>T is 11, above the 10 of C"),
    (GOOD[:3] + ["3p\t+\t1\t1\t10\t10\t1\t22\t12\t1"] + GOOD[4:], 1, "line 4: G>A is 12, above the 10 of G"),
    (GOOD[:3], 1, "holds no 3p rows"),
    ([HEAD] + GOOD[3:], 1, "holds no 5p rows"),
    (GOOD, 2, "--pileup-damage-positions 2 needs positions beyond it for the tail, and the largest Pos is 2"),
    (GOOD, 20, "the largest Pos is 2"),
    (GOOD, 0, "--pileup-damage-positions 0: 1..254"),
    (GOOD, 255, "--pileup-damage-positions 255: 1..254"),
])
def test_profile_errors(lines, k, words):
    from mapdamage_amd import pileup
    with pytest.raises(pileup.ProfileError) as error:
        pileup.parse_damage_profile(lines, k, "dir/misincorporation.txt")
    assert words in str(error.value) and ("dir/misincorporation.txt" in str(error.value) or "--pileup-damage-positions" in str(error.value))
    with pytest.raises(ValueError):
        DR.profile("\n".join(lines), k)
    assert pileup.parse_damage_profile(GOOD, 1).ends == [[(3, 10, 0.3), (1, 10, 0.1)], [(2, 10, 0.2), (1, 10, 0.1)]]


# ---------------------------------------------------------------------- the table
def test_table_is_the_brute_force_s():
    from mapdamage_amd import pileup
    for k in (5, 20):
        p = pileup.parse_damage_profile(TEXT.split("\n"), k)
        table = pileup.damage_likelihood_table(p)
        assert table.shape == (2, k + 1, 94, 9) and table.dtype == np.int64
        assert table.tolist() == DR.table(*DR.profile(TEXT, k))
        # every probability is at least e / 3: the plain table's bound
        assert int(np.abs(table).max()) == 377699653 == abs(GR.TABLE[93][2]) and int(np.abs(table).max()) * 2**31 < 2**63 and (table <= 0).all()


def test_table_without_damage_is_the_plain_table():
    from mapdamage_amd import pileup
    zero = pileup.damage_likelihood_table(pileup.parse_damage_profile(DR.misincorporation_text([(0, 50)] * 8, [(0, 60)] * 8).split("\n"), 3))
    assert zero.shape == (2, 4, 94, 9)
    for q in range(94):
        hom, het, no = GR.TABLE[q]
        assert DR.channel_terms(0.0, q) == pileup.damage_terms(0.0, q) == [hom, het, no, hom, het, no, het, no, no]
        assert all(zero[end, row, q].tolist() == [hom, het, no, hom, het, no, het, no, no] for end in range(2) for row in range(4))


def test_table_rows_by_hand():
    from mapdamage_amd import pileup
    unit = 2.0**24
    # r = 0.3, q = 30: e = 0.001, Pss = 0.7 * 0.999 + 0.3 * 0.001 / 3 = 0.6994, Pst = 0.3 * 0.999 + 0.7 * 0.001 / 3 = 0.2999333...
    e = 0.001
    want = [math.log(0.6994), math.log(0.6994 / 2 + e / 6), math.log(e / 3), math.log(0.999), math.log((0.29970 + 0.0007 / 3) / 2 + 0.4995),
            math.log(0.29970 + 0.0007 / 3), math.log(0.4995 + e / 6), math.log((0.29970 + 0.0007 / 3) / 2 + e / 6), math.log(e / 3)]
    got = pileup.damage_terms(0.3, 30)
    assert all(abs(g - w * unit) <= 1 for g, w in zip(got, want)), (got, [w * unit for w in want])
    assert got == [-5998399, -17619485, -134324558, -16786, -7241110, -20203040, -11640269, -31813485, -134324558]      # (logarithms to 50 digits)
    # r = 1 (every C read as T): observed C is an error whatever the genotype; observed T under CC is as good as under TT
    full = pileup.damage_terms(1.0, 20)
    assert full[0] == full[1] == full[2] == GR.TABLE[20][2] and full[5] == full[4] == full[3] == GR.TABLE[20][0]
    # q = 0 and 1, e = 0.75: every probability is a quarter
    for q in (0, 1):
        assert all(abs(x - round(math.log(0.25) * unit)) <= 1 for r in (0.0, 0.3, 1.0) for x in pileup.damage_terms(r, q))


def test_table_is_monotone_in_the_rate():
    from mapdamage_amd import pileup
    steps = [0.0, 1e-6, 0.001, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.0]
    for q in (2, 10, 20, 30, 41, 93):
        rows = [pileup.damage_terms(r, q) for r in steps]
        for lo, hi in zip(rows, rows[1:]):
            assert hi[0] <= lo[0] and hi[1] <= lo[1] and hi[5] >= lo[5] and hi[4] >= lo[4] and hi[7] >= lo[7]       # log Pss falls, log Pst rises
            assert (hi[2], hi[3], hi[6], hi[8]) == (lo[2], lo[3], lo[6], lo[8])                  # the terms without the rate stay
        assert rows[-1][0] < rows[0][0] and rows[-1][5] > rows[0][5]
        assert all(rows[k + 1][0] < rows[k][0] and rows[k + 1][5] > rows[k][5] for k in range(2, len(steps) - 1))


def test_channel_form_is_the_model():
    """The nine terms placed by genotype are log(P(b|a1)/2 + P(b|a2)/2) of the error model's table for every observed base and
    genotype: the brute force's own two forms against each other."""
    for ct, ga in ((0.0, 0.0), (0.3, 0.0), (0.0, 0.25), (0.31, 0.02), (1.0, 1.0)):
        for q in (0, 2, 20, 30, 93):
            for obs in range(4):
                ten, real = DR.ten_terms(obs, q, ct, ga), DR.real_terms(obs, q, ct, ga)
                assert all(abs(t - x * 2**24) <= 1 for t, x in zip(ten, real)), (obs, q, ct, ga, ten, real)
    assert sorted({DR.which_term(b, a1, a2) for b in (C, G) for a1, a2 in DR.PAIRS}) == [0, 1, 2]
    assert sorted({DR.which_term(b, a1, a2) for b in (A, T) for a1, a2 in DR.PAIRS}) == [3, 4, 5, 6, 7, 8]


# ---------------------------------------------------------------------- the host program
@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("pileup_gld") / "pileup_gld_host"
    subprocess.check_call(["g++", *request.param, "-I", CSRC, os.path.join(ROOT, "tests", "pileup_gld_host.cpp"), "-o", str(exe)])
    tables = {}

    def run(part, text, rows):
        out = subprocess.run([str(exe)], input=(part + "\n" + "\n".join(text) + "\n").encode(), capture_output=True, timeout=300)
        assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
        assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
        lines = out.stdout.decode().split("\n")
        assert lines[-2] == "OK" and len(lines) == rows + 2
        return lines[:rows]

    def sums(records, n_libraries, lengths, sites, d5, d3, k5=0, k3=0, min_qual=0, packed=False, noqual=30, single_strand=False, alleles=None):
        """-> (counters [sites][12], sums: a list of 20 per site, gl [sites][10], best, bases, the two counts)"""
        key = (tuple(DR.rates(d5)), tuple(DR.rates(d3)))
        if key not in tables:
            tables[key] = " ".join(str(x) for end in DR.table(d5, d3) for row in end for nine in row for x in nine)
        text = batch_text(records, n_libraries, lengths, k5, k3, min_qual, packed)
        text.append("%d %d %d %d %d" % (noqual, int(single_strand), len(sites), int(alleles is not None), len(d5)))
        text.append(" ".join(str(int(x)) for x in site_offsets(sites, len(lengths))))
        text += ["%d" % p + ("" if alleles is None else " %d %d" % tuple(PR.BASES.index(a) for a in alleles[g])) for g, (_, p) in enumerate(sites)]
        text.append(tables[key])
        lines = run("sums", text, len(sites) + 1)
        rows = [[int(x) for x in line.split()] for line in lines[:-1]]
        assert all(len(row) == 12 + 20 + 10 + 2 for row in rows)
        counts = dict(zip(("added", "without_qualities"), (int(x) for x in lines[-1].split())))
        return (np.array([row[:12] for row in rows], np.uint32).reshape(-1, 12), [row[12:32] for row in rows],
                np.array([row[32:42] for row in rows], np.int64).reshape(-1, 10), [row[42] for row in rows], [row[43] for row in rows], counts)

    def finish(rows, single_strand=False):
        """rows of (20 sums, 8 counters, ref, alt) -> [(the ten values, best, bases)]"""
        text = ["%d %d" % (len(rows), int(single_strand))] + [" ".join(map(str, list(s) + list(c) + [r, a])) for s, c, r, a in rows]
        out = [[int(x) for x in line.split()] for line in run("finish", text, len(rows))]
        return [(row[:10], row[10], row[11]) for row in out]

    class Host:
        pass
    h = Host()
    h.sums, h.finish = sums, finish
    return h


def against_the_rule(host, records, n_libraries, lengths, sites, d5, d3, k5=0, k3=0, min_qual=0, packed=False, noqual=30, single_strand=False, alleles=None):
    counters, sums, gl, best, bases, counts = host.sums(records, n_libraries, lengths, sites, d5, d3, k5, k3, min_qual, packed, noqual, single_strand, alleles)
    want_counters, _ = PR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual)
    want_sums, want_counts = DR.brute(records, n_libraries, lengths, sites, DR.rates(d5), DR.rates(d3), k5, k3, min_qual, noqual)
    want_gl, want_best, want_bases = DR.all_likelihoods(want_sums, want_counters, alleles, single_strand)
    assert (counters == want_counters).all()
    assert sums == want_sums, [(sites[g], sums[g], want_sums[g]) for g in range(len(sites)) if sums[g] != want_sums[g]][:3]
    assert (gl == want_gl).all() and best == want_best and bases == want_bases and counts == want_counts
    assert (gl <= 0).all() and all(gl[g, best[g]] == 0 for g in range(len(sites)))
    assert counts["added"] == int(want_counters[:, :8].sum())                       # a pair adds exactly where it adds to a base counter
    return want_sums, want_gl, want_best, want_bases, want_counts


# ---------------------------------------------------------------------- the rule
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
def test_hand_written_records(host, packed):
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(HAND_SITES))]
    for n, (k5, k3, q) in enumerate(HAND_SETTINGS):
        d5, d3 = ((D5_K5, D3_K5), (D5_K20, D3_K20))[n % 2]
        _, _, _, bases, counts = against_the_rule(host, HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, d5, d3, k5, k3, q, packed, noqual=(30, 7)[n % 2],
                                                  single_strand=bool(n % 2), alleles=alleles if n % 3 else None)
    assert counts["added"] == 0                                                     # (windows longer than every read: every base Masked)


def special_records():
    """What the issue lists: reads shorter than K, a one-base read, reverse records, soft clips, an insertion in front of the site,
    sites under D and N, a CIGAR longer than its SEQ (and a SEQ that its clips swallow), records without qualities."""
    return [
        rec(0, 0, 0, 10, [(M, 4)], "CTGA"),                                         # shorter than K: both distances inside the profile
        rec(0x10, 1, 0, 10, [(M, 4)], "CTGA", [40, 20, 10, 2]),
        rec(0, 0, 0, 12, [(M, 1)], "T"),                                            # one base: z5 = z3 = 1
        rec(0x10, 0, 0, 12, [(M, 1)], "A"),
        rec(0, 2, 0, 20, [(S, 3), (M, 6), (S, 2)], "NNNCTTGAANN"[:11]),             # soft clips: the distances start behind them
        rec(0x10, 2, 0, 20, [(H, 2), (S, 1), (M, 6), (S, 4), (H, 1)], "GTCAGATTTTC"),
        rec(0, 0, 0, 30, [(M, 2), (I, 3), (M, 5)], "CTAAACTGAT"),                   # an insertion in front of the sites 32 ..: query bases
        rec(0x10, 1, 0, 30, [(M, 2), (I, 3), (M, 5)], "CTAAACTGAT"),
        rec(0, 0, 0, 40, [(M, 3), (D, 2), (M, 3), (N, 4), (M, 3)], "CTGACTGAC"),    # D and N: no query base, no distance
        rec(0x10, 0, 0, 40, [(M, 3), (D, 2), (M, 3), (N, 4), (M, 3)], "CTGACTGAC"),
        rec(0, 0, 0, 60, [(M, 12)], "CTGACTG"),                                     # a CIGAR longer than its SEQ
        rec(0, 1, 0, 60, [(M, 8), (S, 5)], "CTGACTGACT"),                           # ... whose trailing clip starts inside the bases over sites
        rec(0x10, 1, 0, 60, [(S, 3), (M, 4), (S, 3)], "TGACT"),                     # ... whose clips swallow the SEQ: no query, qs = qe = 0
        rec(0, 1, 0, 72, [(M, 9)], "CTGACTGAC", None),                              # no qualities
        rec(0x10, 2, 0, 72, [(M, 9)], "CTGACTGAC", [0xFF] + [30] * 8),
        rec(0, 0, 0, 85, [(M, 30)], "CTGAC" * 6),                                   # long enough to reach the tail from both ends
        rec(0x10, 0, 0, 85, [(M, 30)], "TCAGG" * 6, [int(x) for x in range(5, 35)]),
    ]


@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
def test_special_records(host, packed):
    records, sites = special_records(), [(0, p) for p in range(5, 120)]
    for (d5, d3), k5, k3, q in (((D5_K5, D3_K5), 0, 0, 0), ((D5_K20, D3_K20), 0, 0, 0), ((D5_K5, D3_K5), 1, 2, 10)):
        _, _, _, bases, counts = against_the_rule(host, records, 3, [200], sites, d5, d3, k5, k3, q, packed, noqual=25)
        assert counts["added"] > 100 and counts["without_qualities"] == 18 - (3 if k5 else 0) * 2


def test_distances_by_hand():
    """The brute force's distances, so that the yardstick is itself held to something."""
    assert DR.distances(0, [(M, 10)], 10, 0) == (1, 10) and DR.distances(0, [(M, 10)], 10, 9) == (10, 1)
    assert DR.distances(0x10, [(M, 10)], 10, 0) == (10, 1) and DR.distances(0x10, [(M, 10)], 10, 9) == (1, 10)
    assert DR.distances(0, [(S, 3), (M, 6), (S, 2)], 11, 3) == (1, 6) and DR.distances(0x10, [(S, 3), (M, 6), (S, 2)], 11, 8) == (1, 6)
    assert DR.distances(0, [(M, 2), (I, 3), (M, 5)], 10, 5) == (6, 5)               # the insertion's three bases count
    assert DR.distances(0, [(M, 1)], 1, 0) == (1, 1)
    assert DR.distances(0, [(M, 8), (S, 5)], 10, 7) == (8, 1)                       # qe = 5: base 7 lies behind it, z3 = -2 is taken as 1
    assert DR.distances(0x10, [(S, 3), (M, 4), (S, 3)], 5, 4) == (1, 5)             # no query: qs = qe = 0


def one_base(host, flag, base, q, d5, d3, pos=100, cigar=None, seq=None, site=None):
    cigar = cigar or [(M, 1)]
    records = [rec(flag, 0, 0, pos, cigar, seq or base, [q] * len(seq or base))]
    _, sums, gl, best, bases, counts = host.sums(records, 1, [500], [(0, pos if site is None else site)], d5, d3)
    assert bases == [1] and counts["added"] == 1
    return sums[0], gl[0].tolist(), best[0]


def test_one_base_by_hand(host):
    """A forward T at quality 30 at z5 = 1 under d5[1] = 0.3, from the formulas; the same base on a reverse record, whose ct is
    d3's."""
    d5 = [(3, 10, 0.3), (0, 10, 0.0)]
    d3 = [(2, 10, 0.2), (0, 10, 0.0)]
    unit = 2**24
    hom, het, no = GR.TABLE[30]
    e = 0.001
    # forward, the read's first base of five: z5 = 1 (ct = 0.3), z3 = 5 (the tail)
    sums, gl, best = one_base(host, 0, "T", 30, d5, d3, cigar=[(M, 5)], seq="TAAAA", site=100)
    pst = 0.3 * (1 - e) + 0.7 * (e / 3)
    assert best == TT and sums[10:] == [0] * 10
    assert gl[CC] == round(math.ldexp(math.log(pst), 24)) - hom                     # term(Pst) - term(1 - e)
    assert abs(gl[CC] / unit - math.log(pst / (1 - e))) < 1e-6 and gl[CC] > (no - hom) // 6     # -1.2 against the plain model's -8.0
    assert gl[CT] == round(math.ldexp(math.log(pst / 2 + (1 - e) / 2), 24)) - hom and abs(gl[CT] / unit - math.log((pst + 1 - e) / 2 / (1 - e))) < 1e-6
    assert gl[AT] == gl[GT] == het - hom and gl[AA] == gl[AG] == gl[GG] == no - hom
    assert gl[AC] == gl[CG] == round(math.ldexp(math.log(pst / 2 + (e / 3) / 2), 24)) - hom
    assert gl[CT] > gl[AT] > gl[CC] > gl[AC] > gl[AA]
    # the same T as the last base: z5 = 5, the tail's rate 0 -> the plain model
    _, gl_far, _ = one_base(host, 0, "T", 30, d5, d3, cigar=[(M, 5)], seq="AAAAT", site=104)
    assert gl_far == [no - hom, no - hom, no - hom, het - hom, no - hom, no - hom, het - hom, no - hom, het - hom, 0]
    # a reverse record, stored T at the stored left end: the molecule's 3' end, z3 = 1, and ct = d3[1] = 0.2
    sums, gl, best = one_base(host, 0x10, "T", 30, d5, d3, cigar=[(M, 5)], seq="TAAAA", site=100)
    pst = 0.2 * (1 - e) + 0.8 * (e / 3)
    assert best == TT and sums[:10] == [0] * 10 and gl[CC] == round(math.ldexp(math.log(pst), 24)) - hom
    # ... and a stored A at the stored right end of a reverse record is the molecule's 5' C>T: ga = d5[1] = 0.3
    _, gl, best = one_base(host, 0x10, "A", 30, d5, d3, cigar=[(M, 5)], seq="CCCCA", site=104)
    pst = 0.3 * (1 - e) + 0.7 * (e / 3)
    assert best == AA and gl[GG] == round(math.ldexp(math.log(pst), 24)) - hom and gl[AG] == round(math.ldexp(math.log(pst / 2 + (1 - e) / 2), 24)) - hom
    assert gl[CC] == gl[TT] == gl[CT] == no - hom
    # an observed C at z5 = 1: CC loses log(Pss / (1 - e)) against nothing — it is still the best, every other genotype gains
    _, gl, best = one_base(host, 0, "C", 30, d5, d3, cigar=[(M, 5)], seq="CAAAA", site=100)
    pss = 0.7 * (1 - e) + 0.3 * (e / 3)
    assert best == CC and gl[TT] == no - round(math.ldexp(math.log(pss), 24)) and gl[CT] == round(math.ldexp(math.log(pss / 2 + (e / 3) / 2), 24)) - round(
        math.ldexp(math.log(pss), 24))


def test_a_zero_profile_is_the_plain_model(host):
    """Through the whole rule: under rates of zero the sums folded to gl are the plain stage's gl (tests/gl_rule.py, to which
    tests/test_pileup_likelihoods.py holds that stage) on the same records."""
    lengths = [400, 1, 0, 150]
    records = random_records(5, 1200, lengths) + special_records()
    sites = sorted({(0, p) for p in range(0, 400, 3)} | {(3, p) for p in range(150)})
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(sites))]
    want_counters, _ = PR.brute(records, 3, lengths, sites, 1, 0, 10)
    plain_sums, plain_counts = GR.brute(records, 3, lengths, sites, 1, 0, 10, 22)
    for single_strand in (False, True):
        counters, sums, gl, best, bases, counts = host.sums(records, 3, lengths, sites, ZERO5, ZERO3, 1, 0, 10, False, 22, single_strand, alleles)
        want_gl, want_best, want_bases = GR.all_likelihoods(plain_sums, want_counters, alleles, single_strand)
        assert (gl == want_gl).all() and best == want_best and bases == want_bases and counts == plain_counts and counts["added"] > 500


@pytest.mark.parametrize("seed,packed", [(1, False), (2, True)])
def test_rule_on_random_records(host, seed, packed):
    lengths = [400, 1, 0, 150]
    records = random_records(seed, 2500, lengths) + [rec(0, 0, 1, 0, [(S, 3), (M, 1)]), rec(0x10, 2, 1, 0, [(EQ, 1), (I, 2)])] + [
        (f, lib, 3, p, c, s, q) for f, lib, _, p, c, s, q in special_records()]
    rng = np.random.default_rng(seed)
    sites = sorted({(0, int(p)) for p in rng.choice(400, 150, replace=False)} | {(1, 0)} | {(3, p) for p in range(150)})
    alleles = [tuple(PR.BASES[int(b)] for b in rng.choice(4, 2, replace=False)) for _ in sites]
    k5, k3, q = [(0, 0, 15), (1, 0, 30)][seed - 1]
    d5, d3 = [(D5_K5, D3_K5), (D5_K20, D3_K20)][seed - 1]
    _, gl, best, bases, counts = against_the_rule(host, records, 3, lengths, sites, d5, d3, k5, k3, q, packed, noqual=25, single_strand=True, alleles=alleles)
    assert counts["added"] > 500 and counts["without_qualities"] > 50 and len(set(best)) >= 8 and 0 in bases and max(bases) >= 5


def test_finish_by_hand(host):
    rng = np.random.default_rng(4)
    rows = []
    for _ in range(40):
        c = [int(x) for x in rng.integers(0, 3, 8)]
        s = [-int(x) for x in rng.integers(0, 10**9, 20)]
        s[:10] = s[:10] if sum(c[:4]) else [0] * 10
        s[10:] = s[10:] if sum(c[4:]) else [0] * 10
        rows.append((s, c, *[(-1, -1), (1, 3), (2, 0), (0, 1)][len(rows) % 4]))
    big = 2**31 - 1
    rows.append(([0] * 10 + [big * GR.TABLE[93][2]] * 9 + [0], [0, 0, 0, 0, 0, 0, 0, big], -1, -1))       # sums as large as the limit allows
    rows.append(([0] * 20, [0] * 8, -1, -1))
    rows.append(([-5] * 10 + [-7] * 10, [1, 0, 0, 0, 0, 1, 0, 0], 3, 1))            # ties: the first genotype
    for single_strand in (False, True):
        got = host.finish(rows, single_strand)
        for (s, c, r, a), one in zip(rows, got):
            assert one == DR.likelihoods(s, c + [0] * 4, None if r < 0 else (PR.BASES[r], PR.BASES[a]), single_strand)
    assert got[-3] == ([big * GR.TABLE[93][2]] * 9 + [0], 9, big) and got[-2] == ([0] * 10, 0, 0) and got[-1] == ([0] * 10, 0, 1)


# ---------------------------------------------------------------------- the emitters
def test_emitters():
    from mapdamage_amd import pileup
    p = pileup.parse_damage_profile(TEXT.split("\n"), 5, "run1/misincorporation.txt")
    text = pileup.damage_profile_text(p)
    assert text == DR.profile_text(D5_K5, D3_K5)
    lines = text.split("\n")
    assert lines[0] == "End\tPosition\tSubstitutions\tBases\tRate" and len(lines) == 1 + 12 + 1
    assert lines[1] == "5p\t1\t309\t997\t%s" % ("%.15g" % (309 / 997)) and lines[6].startswith("5p\t>5\t") and lines[7].startswith("3p\t1\t274\t1013\t")
    assert lines[12] == "3p\t>5\t%d\t%d\t%s" % (sum(s for s, _ in ROWS3[5:]), 1013 * 25, "%.15g" % (sum(s for s, _ in ROWS3[5:]) / (1013 * 25)))
    line = pileup.damage_profile_log_line(p)
    assert line == DR.log_line("run1/misincorporation.txt", D5_K5, D3_K5)
    assert line == "Pileup damage profile: run1/misincorporation.txt, 5 positions; 5p C>T 0.30993 at position 1, tail %.6g; 3p G>A 0.270484, tail %.6g" % (
        D5_K5[-1][2], D3_K5[-1][2])


# ---------------------------------------------------------------------- the command line
@pytest.fixture()
def files(tmp_path):
    (tmp_path / "plain.txt").write_text("# sites\nchr1\t5\nchr1\t9\n")
    (tmp_path / "in.bam").write_bytes(b"")
    (tmp_path / "misincorporation.txt").write_text(TEXT)
    (tmp_path / "short.txt").write_text(DR.misincorporation_text(ROWS5[:10], ROWS3[:10]))
    (tmp_path / "bad.txt").write_text("\n".join(GOOD[:2] + ["5p\t+\t2\t1\t10\t10\t1\t22\t1\t11"] + GOOD[3:]) + "\n")
    return tmp_path


@pytest.mark.parametrize("extra,words", [
    (["--pileup-sites", "{plain}", "--pileup-damage-profile", "{mis}"], "--pileup-damage-profile needs --pileup-likelihoods"),
    (["--pileup-damage-profile", "{mis}"], "--pileup-damage-profile needs --pileup-likelihoods"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-positions", "5"], "--pileup-damage-positions needs --pileup-damage-profile"),
    (["--pileup-damage-positions", "5"], "--pileup-damage-positions needs --pileup-damage-profile"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--single-stranded"],
     "--pileup-damage-profile cannot be combined with --single-stranded"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--pileup-damage-positions", "3", "--single-stranded"],
     "--pileup-damage-profile cannot be combined with --single-stranded"),
    (["-i", "{dir}/in.bam", "--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{dir}/in.bam"], "in.bam is the input file"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{dir}/none.txt"], "none.txt: [Errno 2]"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{bad}"], "bad.txt, line 3: C>T is 11, above the 10 of C"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{short}"], "--pileup-damage-positions 20 needs positions beyond it"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--pileup-damage-positions", "30"], "the largest Pos is 30"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--pileup-damage-positions", "0"],
     "--pileup-damage-positions 0: 1..254"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--pileup-damage-positions", "255"],
     "--pileup-damage-positions 255: 1..254"),
    # every restriction of --pileup-likelihoods stands
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "-Q", "20"], "--pileup-likelihoods cannot be combined with -Q 20"),
    (["--pileup-likelihoods", "--pileup-damage-profile", "{mis}"], "--pileup-likelihoods needs --pileup-sites"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--gpus", "2"], "--pileup-sites cannot be combined with --gpus 2"),
    (["--pileup-sites", "{plain}", "--pileup-likelihoods", "--pileup-damage-profile", "{mis}", "--host-decode"], "not with --host-decode"),
])
def test_argument_errors(capsys, files, extra, words):
    from mapdamage_amd.main import parse_args
    names = dict(plain=files / "plain.txt", mis=files / "misincorporation.txt", short=files / "short.txt", bad=files / "bad.txt", dir=files)
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + [e.format(**names) for e in extra])
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_arguments_that_pass(files):
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--pileup-sites", str(files / "plain.txt"), "--pileup-likelihoods", "--pileup-damage-profile", str(files / "misincorporation.txt")])
    assert o.pileup_damage_positions == 20 and (o.pileup_damage_profile_rows.ends[0], o.pileup_damage_profile_rows.ends[1]) == (D5_K20, D3_K20)
    o = parse_args(BASE + ["--pileup-sites", str(files / "plain.txt"), "--pileup-likelihoods", "--pileup-damage-profile", str(files / "short.txt"),
                           "--pileup-damage-positions", "9", "--pileup-mask-ends", "1,0", "--pileup-noqual-quality", "20"])
    assert o.pileup_damage_positions == 9 and len(o.pileup_damage_profile_rows.ends[1]) == 10
    o = parse_args(BASE + ["--pileup-sites", str(files / "plain.txt"), "--pileup-likelihoods"])
    assert o.pileup_damage_profile is None and o.pileup_damage_positions is None and getattr(o, "pileup_damage_profile_rows", None) is None
