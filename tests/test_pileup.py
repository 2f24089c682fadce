"""--pileup-sites, the parts that need no GPU: the rule (mapdamage_amd/csrc/mdx_pileup_key.h compiled for the host as the
stand-alone program tests/pileup_key_host.cpp, once more under AddressSanitizer and UBSan, against the brute force of
tests/pileup_rule.py), the parser of the sites file, the command line's argument errors and the emitters of
mapdamage_amd/pileup.py.  The device stage: tests/test_gpu_pileup.py."""

import os
import subprocess

import numpy as np
import pytest

from tests import mask_rule as MR
from tests import pileup_rule as PR
from tests.dup_rule import columns
from tests.test_depth import HAND as DEPTH_HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
M, I, D, N, S, H, P, EQ, X = range(9)
UNKNOWN = 0xFFFF
NIBBLE_OF = {"A": 1, "C": 2, "T": 4, "G": 8}
MODES = {"none": 0, "random": 1, "majority": 2}


def rec(flag, lib, tid, pos, cigar, seq=None, qual="default"):
    """A record of the rule: SEQ ``ACGTACGT...`` of the CIGAR's query length and quality 30 everywhere unless given."""
    n = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
    seq = "".join("ACGT"[(k + pos) % 4] for k in range(n)) if seq is None else seq
    return (flag, lib, tid, pos, cigar, seq, [30] * len(seq) if isinstance(qual, str) else qual)


# ---------------------------------------------------------------------- the hand-written records and sites (the GPU test runs them too)
HAND_LENGTHS = [500, 300]
HAND_LIBRARIES = 3
HAND_RECORDS = [
    rec(0, 0, 0, 10, [(M, 30), (I, 2), (M, 30)]),                                 # sites at its first and last base, one outside either, around the I
    rec(0, 1, 0, 100, [(M, 20), (D, 5), (M, 20)]),                                # under D
    rec(0, 2, 0, 200, [(M, 10), (D, 3), (N, 4), (EQ, 10)]),                       # under D, under N, under =
    rec(0x10, 0, 0, 300, [(S, 5), (M, 50), (H, 5)]),                              # reverse, behind a leading S
    rec(0, 0, 0, 360, [(H, 3), (S, 2), (M, 10)]),                                 # behind a leading H and S
    rec(0, 0, 0, 440, [(M, 5), (EQ, 5), (X, 5)]),                                 # = and X
    rec(0, 1, 0, 380, [(M, 10)], qual=None),                                      # no qualities: never LowQual
    rec(0, 0, 0, 395, [(M, 4)], "ACGT", [20, 19, 20, 0]),                         # a quality exactly Q and exactly Q - 1 (Q = 20)
    rec(0x10, 2, 0, 395, [(M, 4)], "TTGA", [19, 20, 21, 93]),
    rec(0, 0, 0, 405, [(M, 6)], "ANGRT="),                                        # symbols that are no base
    rec(0, 0, 0, 0, [(M, 5)]),                                                    # the first base of a sequence
    rec(0, 0, 0, 480, [(M, 20)]),                                                 # ... and the last
    rec(0, 0, 1, 0, [(M, 300)], "ACGT" * 75),                                     # a whole sequence
    rec(0x10, 1, 1, 299, [(M, 1)], "G"),
    rec(0x10, 0, 0, 420, [(M, 3)], "CAT"),                                        # shorter than the windows
    rec(0, 0, 0, 420, [(S, 1), (M, 3), (S, 2)], "GCATGG"),
    rec(0, 0, 0, 456, [(M, 5), (P, 2), (I, 1), (S, 0), (M, 5)]),
    rec(0, 0, 0, 403, [(D, 3), (M, 10)]),                                         # D first
    rec(0x10, 0, 0, 10, [(M, 20)], "T" * 20),                                     # over the first record's sites, the other strand
    rec(0x1 | 0x20 | 0x40, 0, 0, 10, [(M, 20)], "C" * 20),                        # a paired record is a record
] + [rec(*r) for r, kind, _ in DEPTH_HAND if kind != PR.COUNTED]                  # every OUTSIDE and IGNORED case of --depth
HAND_SITES = sorted({(0, p) for p in (0, 4, 5, 9, 10, 11, 29, 30, 39, 40, 41, 50, 55, 69, 70, 99, 100, 119, 120, 124, 125, 144, 145, 199, 200, 209, 210, 212, 213, 216, 217,
                                      226, 227, 299, 300, 301, 348, 349, 350, 359, 360, 369, 370, 380, 389, 395, 396, 397, 398, 403, 405, 406, 407, 408, 409, 410,
                                      412, 420, 421, 422, 423, 440, 444, 445, 449, 450, 454, 455, 456, 460, 461, 465, 466, 480, 485, 490, 499)}
                    | {(1, p) for p in (0, 1, 5, 150, 298, 299)})
# (k5, k3, Q): no window, one base at either end, windows that overlap in the short reads, windows longer than every read
HAND_SETTINGS = [(0, 0, 0), (0, 0, 20), (1, 0, 20), (0, 1, 0), (3, 2, 20), (2, 2, 21), (40, 30, 0), (255, 255, 20)]


def batch_text(records, n_libraries, lengths, k5, k3, min_qual, packed, cigar_off=None, n_cigar=None, seq_off=None, n_bases=None):
    """The columns of a batch as the host program reads them."""
    flag, lib, tid, pos, off, cigar = columns([r[:5] for r in records])
    off = off if cigar_off is None else np.asarray(cigar_off, np.uint32)
    soff = np.zeros(len(records) + 1, np.int64)
    soff[1:] = np.cumsum([len(r[5]) for r in records])
    soff = soff if seq_off is None else np.asarray(seq_off, np.int64)
    symbols, quals = [], []
    has_qual = any(r[6] is not None for r in records)
    for r in records:
        for s in r[5]:
            if isinstance(s, str):
                symbols.append(NIBBLE_OF.get(s, 0) if packed else ord(s))
            else:
                assert packed
                symbols.append(int(s))
        quals += list(r[6]) if r[6] is not None else [0xFF] * len(r[5])
    held = len(symbols)
    text = ["%d %d %d %d %d %d %d %d %d %d %d %d" % (len(lengths), n_libraries, len(records), len(cigar), len(cigar) if n_cigar is None else n_cigar, held,
                                                     held if n_bases is None else n_bases, int(packed), int(has_qual), k5, k3, min_qual),
            " ".join(str(int(x)) for x in lengths)]
    text += ["%d %d %d %d" % row for row in zip(flag.tolist(), lib.tolist(), tid.tolist(), pos.tolist())]
    text += [" ".join(str(int(x)) for x in off), " ".join(str(int(x)) for x in cigar), " ".join(str(int(x)) for x in soff), " ".join(map(str, symbols))]
    if has_qual:
        text.append(" ".join(map(str, quals)))
    return text


def site_offsets(sites, n_contig):
    off = np.zeros(n_contig + 1, np.int64)
    off[1:] = np.cumsum(np.bincount([t for t, _ in sites], minlength=n_contig))
    return off


@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def host(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("pileup_key") / "pileup_key_host"
    subprocess.check_call(["g++", *request.param, "-I", CSRC, os.path.join(ROOT, "tests", "pileup_key_host.cpp"), "-o", str(exe)])

    def run(part, text, rows):
        out = subprocess.run([str(exe)], input=(part + "\n" + "\n".join(text) + "\n").encode(), capture_output=True, timeout=300)
        assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
        assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
        lines = out.stdout.decode().split("\n")
        assert lines[-2] == "OK" and len(lines) == rows + 2
        return lines[:rows]

    def pileup(records, n_libraries, lengths, sites, k5=0, k3=0, min_qual=0, packed=False, mode="random", seed=0, min_depth=1, single_strand=False,
               alleles=None, **layout):
        text = batch_text(records, n_libraries, lengths, k5, k3, min_qual, packed, **layout)
        text.append("%d %d %d %d %d %d" % (len(sites), int(alleles is not None), MODES[mode], seed, min_depth, int(single_strand)))
        text.append(" ".join(str(int(x)) for x in site_offsets(sites, len(lengths))))
        text += ["%d" % p + ("" if alleles is None else " %d %d" % tuple(PR.BASES.index(a) for a in alleles[g])) for g, (_, p) in enumerate(sites)]
        lines = run("pileup", text, len(sites) + 1)
        rows = [line.split() for line in lines[:-1]]
        counts = dict(zip(("counted", "outside", "over_a_site", "pairs"), (int(x) for x in lines[-1].split())))
        return np.array([[int(x) for x in row[:12]] for row in rows], np.uint32).reshape(-1, 12), [row[12] for row in rows], counts

    def masked(records, n_libraries, lengths, k5, k3, packed=False):
        lines = run("masked", batch_text(records, n_libraries, lengths, k5, k3, 0, packed), len(records))
        return [(int(line.split()[0]), {int(x) for x in line.split()[1:]}) for line in lines]

    def calls(rows, mode, seed, min_depth, single_strand):
        text = ["%d %d %d %d %d" % (len(rows), MODES[mode], seed, min_depth, int(single_strand))]
        text += [" ".join(map(str, list(c) + [t, p, r, a])) for c, t, p, r, a in rows]
        return run("calls", text, len(rows))

    class Host:
        pass
    h = Host()
    h.pileup, h.masked, h.calls = pileup, masked, calls
    return h


# ---------------------------------------------------------------------- the rule
def test_the_yardstick_by_hand():
    """A few sites of the table worked out by hand, so that the brute force is itself held to something."""
    got, counts = PR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, 0, 0, 20)
    row = lambda t, p: dict((PR.NAMES[q], int(n)) for q, n in enumerate(got[HAND_SITES.index((t, p))]) if n)
    assert row(0, 9) == {} and row(0, 70) == {}                                 # one base outside either end
    assert row(0, 10) == {"G+": 1, "T-": 1, "C+": 1}                            # pos 10: "ACGT"[(0 + 10) % 4]; T x 20 reverse; the paired C
    assert row(0, 39) == {"T+": 1} and row(0, 40) == {"G+": 1}                  # around the I: SEQ 29 is T, the I takes 30 and 31, SEQ 32 is G
    assert row(0, 69) == {"T+": 1}                                              # SEQ 61: "ACGT"[(61 + 10) % 4]
    assert row(0, 120) == {"Deletions": 1} and row(0, 124) == {"Deletions": 1} and row(0, 125) == {"A+": 1}
    assert row(0, 210) == {"Deletions": 1} and row(0, 213) == {} and row(0, 216) == {} and row(0, 217) == {"G+": 1}
    assert row(0, 300) == {"C-": 1} and row(0, 349) == {"G-": 1}                # behind 5 S: SEQ 5 and SEQ 54
    assert row(0, 360) == {"G+": 1}                                             # behind H and S: SEQ 2
    assert row(0, 380) == {"A+": 1}                                             # no qualities: counted under Q = 20
    assert row(0, 395) == {"A+": 1, "LowQual": 1} and row(0, 396) == {"LowQual": 1, "T-": 1}
    assert row(0, 397) == {"G+": 1, "G-": 1} and row(0, 398) == {"LowQual": 1, "A-": 1}
    # "ANGRT=" at 405 over the D 3, M 10 of 403, whose M begins at 406 with "ACGT"[403 % 4]
    assert row(0, 405) == {"A+": 1, "Deletions": 1} and row(0, 406) == {"Other": 1, "T+": 1} and row(0, 408) == {"Other": 1, "C+": 1} and row(0, 410) == {"Other": 1, "T+": 1}
    assert row(1, 299) == {"T+": 1, "G-": 1} and row(1, 0) == {"A+": 1}
    assert counts["outside"] == sum(1 for _, k, _ in DEPTH_HAND if k == PR.OUTSIDE)
    # the windows: one base at the 5' end of a forward and of a reverse record
    got, _ = PR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, 1, 0, 0)
    row = lambda t, p: dict((PR.NAMES[q], int(n)) for q, n in enumerate(got[HAND_SITES.index((t, p))]) if n)
    assert row(0, 300) == {"C-": 1} and row(0, 349) == {"Masked": 1}            # a reverse record's 5' end is its right end
    assert row(0, 360) == {"Masked": 1} and row(0, 369) == {"T+": 1}


@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
def test_hand_written_records(host, packed):
    for k5, k3, q in HAND_SETTINGS:
        counters, _, counts = host.pileup(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, k5, k3, q, packed)
        want, want_counts = PR.brute(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, k5, k3, q)
        assert (counters == want).all(), (k5, k3, q, [(HAND_SITES[g], counters[g].tolist(), want[g].tolist()) for g in np.flatnonzero((counters != want).any(axis=1))[:5]])
        assert counts == want_counts
    assert want[:, PR.MASKED].sum() > 20 and want_counts["counted"] == 20


def test_nibbles_of_the_packed_column(host):
    """What only the packed column holds: 0 and 15 for a symbol that is no base, the complemented nibbles of MDX_SEQ_4BITQ."""
    records = [(0, 0, 0, 10, [(M, 16)], list(range(16)), [30] * 16), (0x10, 0, 0, 10, [(M, 16)], [1, 14, 2, 13, 4, 11, 8, 7] * 2, None)]
    sites = [(0, p) for p in range(8, 28)]
    counters, _, _ = host.pileup(records, 1, [100], sites, packed=True)
    want, _ = PR.brute(records, 1, [100], sites)
    assert (counters == want).all()
    assert want[:, PR.OTHER].sum() == 12 + 8 and want[:, :4].sum() == 4 and want[:, 4:8].sum() == 8
    # base 1 (nibble 1) is A, 2 C, 4 T, 8 G
    at = lambda p: {PR.NAMES[q] for q in np.flatnonzero(counters[sites.index((0, p))])}
    assert at(11) == {"A+", "Other"} and at(12) == {"C+", "C-"} and at(14) == {"T+", "T-"} and at(18) == {"G+", "A-"}


def test_clamped_offsets(host):
    """Offsets beyond a column are clamped to it: the record has the operations and the bases that are there, or none."""
    two = [rec(0, 0, 0, 10, [(M, 5)], "ACGTA"), rec(0, 0, 0, 10, [(M, 5), (D, 3), (M, 2)], "CCCCCGG")]
    sites = [(0, p) for p in range(8, 22)]
    # the second record's CIGAR cut to M 5 by the declared size; its SEQ cut to 3 bases: sites beyond them are Other
    counters, _, counts = host.pileup(two, 1, [100], sites, cigar_off=[0, 1, 9], n_cigar=2, seq_off=[0, 5, 99], n_bases=8)
    cut = [two[0], (0, 0, 0, 10, [(M, 5)], "CCC", [30] * 3)]
    want, want_counts = PR.brute(cut, 1, [100], sites)
    assert (counters == want).all() and counts == want_counts and want[:, PR.OTHER].sum() == 2
    # offsets behind their successors: no operation, so outside; no base, so Other
    counters, _, counts = host.pileup(two, 1, [100], sites, cigar_off=[3, 1, 4], seq_off=[7, 12, 2])
    assert counts == dict(counted=1, outside=1, over_a_site=1, pairs=10)
    assert counters[:, PR.DELETIONS].sum() == 3 and counters[:, PR.OTHER].sum() == 7 and counters[:, :8].sum() == 0
    # ... and an offset in front of its record's: the bases that lie there
    counters, _, counts = host.pileup(two, 1, [100], sites, cigar_off=[3, 1, 4], seq_off=[7, 2, 12])
    want, _ = PR.brute([(0, 0, 0, 10, two[1][4], "GTACCCCCGG", [30] * 10)], 1, [100], sites)
    assert (counters == want).all() and counters[:, :8].sum() == 7
    counters, _, counts = host.pileup(two, 1, [100], sites, cigar_off=[5, 7, 9], n_cigar=4)
    assert counts == dict(counted=0, outside=2, over_a_site=0, pairs=0) and not counters.any()


def random_records(seed, n, lengths):
    from tests.test_depth import random_records as depth_records
    rng = np.random.default_rng(seed + 1000)
    out = []
    for flag, lib, tid, pos, cigar in depth_records(seed, n, lengths):
        cigar = [(op, ln % 12) for op, ln in cigar]
        n_seq = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
        if rng.random() < 0.05:
            n_seq = max(0, n_seq + int(rng.integers(-3, 4)))                      # (a SEQ that is not the CIGAR's)
        seq = "".join(rng.choice(list("ACGTACGTACGTNR="), n_seq))
        qual = None if rng.random() < 0.2 else [int(x) for x in rng.integers(0, 42, n_seq)]
        out.append((flag, lib, tid, pos, cigar, seq, qual))
    return out


@pytest.mark.parametrize("seed,packed", [(1, False), (2, True)])
def test_rule_on_random_records(host, seed, packed):
    lengths = [400, 1, 0, 150]
    records = random_records(seed, 2500, lengths) + [rec(0, 0, 1, 0, [(S, 3), (M, 1)]), rec(0x10, 2, 1, 0, [(EQ, 1), (I, 2)])]
    rng = np.random.default_rng(seed)
    sites = sorted({(0, int(p)) for p in rng.choice(400, 150, replace=False)} | {(1, 0)} | {(3, p) for p in range(150)})
    k5, k3, q = [(2, 3, 15), (5, 0, 30)][seed - 1]
    counters, _, counts = host.pileup(records, 3, lengths, sites, k5, k3, q, packed)
    want, want_counts = PR.brute(records, 3, lengths, sites, k5, k3, q)
    assert (counters == want).all(), np.flatnonzero((counters != want).any(axis=1))[:10]
    assert counts == want_counts and counts["counted"] > 300 and counts["outside"] > 300 and counts["pairs"] > counts["over_a_site"] > 100
    assert all(want[:, c].sum() > 10 for c in range(12))


# ---------------------------------------------------------------------- masking: the windows of --mask-ends all
@pytest.mark.parametrize("k5,k3", [(1, 0), (0, 1), (3, 5), (255, 2)])
def test_masked_bases_are_those_of_mask_ends(host, k5, k3):
    rng = np.random.default_rng(k5 * 7 + k3)
    records, want = [], []
    for _ in range(300):
        clip = lambda: [[], [(S, int(rng.integers(1, 6)))], [(H, int(rng.integers(1, 6)))], [(S, 2), (H, 3)]][rng.integers(0, 4)]
        lead, trail = clip(), clip()
        cigar = lead[::-1] + [(M, int(rng.integers(1, 12))), (I, int(rng.integers(0, 3))), (D, int(rng.integers(0, 3))), (M, int(rng.integers(0, 9)))] + trail
        n_seq = sum(ln for op, ln in cigar if op in (M, I, S))
        flag = int(rng.choice((0, 0x10)))
        body, _ = MR.apply(MR.make_record([("MIDNSHP=X"[op], ln) for op, ln in cigar], "A" * n_seq, flag=flag), k5, k3, MR.ALL)
        want.append({b for b, nib in enumerate(MR.decode(body)["nibbles"][:n_seq]) if nib == 15})
        records.append((flag, 0, 0, 5, cigar, "A" * n_seq, [30] * n_seq))
    got = host.masked(records, 1, [100], k5, k3)
    assert [kind for kind, _ in got] == [PR.COUNTED] * len(records)
    assert [s for _, s in got] == want == [PR.masked_set(r[0], r[4], len(r[5]), k5, k3) for r in records]
    assert sum(map(len, want)) >= 300


# ---------------------------------------------------------------------- the call
def test_z_of_three_sites():
    assert PR.z_of(0, 0, 0) == 0xE220A8397B1DCDAF                # (splitmix64's first output for the seed 0)
    assert PR.z_of(1, 2, 3) == 0x12E80FFCFBBBD251
    assert PR.z_of(2**64 - 1, 24, 155270559) == 0x0D10EDE0E87A318B


def row12(plus=(0, 0, 0, 0), minus=(0, 0, 0, 0), rest=(0, 0, 0, 0)):
    return list(plus) + list(minus) + list(rest)


def test_calls_by_hand(host):
    z = PR.z_of(7, 1, 100)
    cases = [
        # (counters, ref, alt, mode, min_depth, single strand) -> call
        ((row12((0, 0, 0, 0)), -1, -1, "random", 1, False), "N"),                                  # nothing eligible
        ((row12((0, 0, 1, 0)), -1, -1, "random", 1, False), "G"),                                  # a total of 1
        ((row12((0, 0, 0, 0), (0, 1, 0, 0)), -1, -1, "majority", 1, False), "C"),
        ((row12((0, 0, 1, 0)), -1, -1, "random", 2, False), "N"),                                  # --pileup-min-depth
        ((row12((1, 0, 0, 0), (1, 0, 0, 0)), -1, -1, "random", 2, False), "A"),
        ((row12((5, 0, 0, 0), (0, 0, 0, 9), (7, 7, 7, 7)), -1, -1, "majority", 1, False), "T"),       # Deletions .. Masked are not eligible
        ((row12((5, 3, 0, 0), (0, 0, 0, 9)), 0, 1, "majority", 1, False), "A"),                    # alleles restrict: T is not eligible
        ((row12((0, 0, 4, 0), (0, 0, 0, 9)), 0, 1, "random", 1, False), "N"),
        ((row12((3, 3, 3, 3)), -1, -1, "majority", 1, False), "ACGT"[z % 4]),                      # ties: number z % k of them
        ((row12((3, 0, 3, 0), (0, 0, 0, 1)), -1, -1, "majority", 1, False), "AG"[z % 2]),
        ((row12((2, 0, 0, 0), (0, 0, 0, 2)), 3, 0, "majority", 1, False), "AT"[z % 2]),
        ((row12((1, 2, 3, 4)), -1, -1, "random", 1, False), "ACCGGGTTTT"[z % 10]),                 # the cumulative count that exceeds z % total
        ((row12((0, 5, 0, 5), (0, 1, 0, 0)), 1, 3, "random", 1, True), "C"),                       # C/T: the - strand alone
        ((row12((0, 5, 0, 5), (0, 0, 0, 0)), 3, 1, "random", 1, True), "N"),
        ((row12((1, 0, 0, 0), (0, 0, 5, 5)), 2, 0, "random", 1, True), "A"),                       # G/A: the + strand alone
        ((row12((1, 0, 0, 0), (0, 0, 5, 0)), 0, 2, "majority", 1, True), "A"),
        ((row12((1, 0, 0, 0), (0, 9, 0, 0)), 0, 1, "majority", 1, True), "C"),                     # a transversion: both strands
        ((row12((1, 0, 0, 0), (0, 9, 0, 0)), 0, 1, "majority", 1, False), "C"),
    ]
    for (row, ref, alt, mode, min_depth, ss), want in cases:
        alleles = None if ref < 0 else (PR.BASES[ref], PR.BASES[alt])
        assert PR.call(row, mode, 7, 1, 100, min_depth, alleles, ss) == want, (row, ref, alt, mode)
        assert host.calls([(row, 1, 100, ref, alt)], mode, 7, min_depth, ss) == [want], (row, ref, alt, mode)


@pytest.mark.parametrize("mode,alleles,single_strand,min_depth", [("random", False, False, 1), ("majority", False, False, 3), ("random", True, True, 1),
                                                                   ("majority", True, True, 2), ("random", True, False, 5)])
def test_ten_thousand_random_rows(host, mode, alleles, single_strand, min_depth):
    rng = np.random.default_rng(len(mode) + 2 * alleles + 4 * single_strand)
    rows = []
    for _ in range(10_000):
        top = int(rng.choice((1, 2, 3, 8, 2**31 - 1)))
        counters = [int(x) for x in rng.integers(0, top + 1, 12)]
        if rng.random() < 0.3:
            for q in rng.choice(8, 6, replace=False):
                counters[q] = 0
        ref, alt = (int(x) for x in rng.choice(4, 2, replace=False)) if alleles else (-1, -1)
        rows.append((counters, int(rng.integers(0, 2**31 - 1)) if rng.random() < 0.1 else int(rng.integers(0, 30)), int(rng.integers(0, 2**31 - 1)), ref, alt))
    seed = int(rng.integers(0, 2**63)) * 2 + 1
    got = host.calls(rows, mode, seed, min_depth, single_strand)
    want = [PR.call(c, mode, seed, t, p, min_depth, None if r < 0 else (PR.BASES[r], PR.BASES[a]), single_strand) for c, t, p, r, a in rows]
    assert got == want
    assert set(got) == set("ACGTN")


def test_calls_of_the_table(host):
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(HAND_SITES))]
    for mode, seed, ss in (("random", 0, False), ("majority", 5, True), ("none", 0, False)):
        counters, got, _ = host.pileup(HAND_RECORDS, HAND_LIBRARIES, HAND_LENGTHS, HAND_SITES, mode=mode, seed=seed, single_strand=ss, alleles=alleles)
        assert got == PR.calls(counters, HAND_SITES, mode, seed, 1, alleles, ss)
    assert set(got) == {"."}


# ---------------------------------------------------------------------- the sites file
NAMES, LENGTHS = ["chr1", "chrM", "scaf/1:a"], [1000, 16569, 7]


def parse(text, names=NAMES, lengths=LENGTHS):
    from mapdamage_amd import pileup
    return pileup.parse_sites(text.splitlines(True), names, lengths, source="sites.txt")


def test_sites_are_sorted_and_zero_based():
    s = parse("# a panel\nchrM\t16569\tA\tG\trs3\n\nchr1\t10\tC\tT\nscaf/1:a\t1\tG\tT\trs9\nchr1\t2\tT\tA\t\nchrM\t1\tC\tA\trs1\r\n")
    assert s.tid.tolist() == [0, 0, 1, 1, 2] and s.pos.tolist() == [1, 9, 0, 16568, 0] and s.off.tolist() == [0, 2, 4, 5]
    assert s.alleles.tolist() == [[3, 0], [1, 3], [1, 0], [0, 2], [2, 3]] and s.ids == [".", ".", "rs1", "rs3", "rs9"]
    assert s.tid.dtype == np.int32 and s.pos.dtype == np.int32 and s.off.dtype == np.int64 and s.alleles.dtype == np.uint8 and len(s) == 5
    s = parse("chrM\t5\nchr1\t1000\n")
    assert s.alleles is None and s.tid.tolist() == [0, 1] and s.pos.tolist() == [999, 4] and s.ids == [".", "."]


@pytest.mark.parametrize("text,words", [
    ("chr1\n", "sites.txt, line 1: fewer than two columns"),
    ("chr1\t5\nchr1 7\n", "sites.txt, line 2: fewer than two columns"),
    ("chr1\tx\n", "line 1: position 'x' is not an integer"),
    ("chr1\t1.5\n", "line 1: position '1.5' is not an integer"),
    ("chr1\t0\n", "line 1: position 0 is below 1"),
    ("chr1\t-3\n", "line 1: position -3 is below 1"),
    ("#\nchr1\t1001\n", "line 2: position 1001 lies beyond the 1000 bases of sequence 'chr1'"),
    ("chr2\t5\n", "line 1: sequence 'chr2' is not in the input's header"),
    ("chr1\t5\tN\tA\n", "line 1: ref 'N' is not exactly one of A C G T"),
    ("chr1\t5\tA\tac\n", "line 1: alt 'ac' is not exactly one of A C G T"),
    ("chr1\t5\tA\tc\n", "line 1: alt 'c' is not exactly one of A C G T"),
    ("chr1\t5\tA\tA\n", "line 1: ref and alt are both 'A'"),
    ("chr1\t5\tA\n", "line 1: a ref without an alt"),
    ("chr1\t5\tA\tC\nchr1\t6\n", "line 1 has alleles and line 2 has none"),
    ("chr1\t5\n\nchr1\t6\tA\tC\n", "line 3 has alleles and line 1 has none"),
    ("chr1\t5\nchrM\t9\nchr1\t5\n", "lines 1 and 3 name the same site, chr1:5"),
    ("# nothing\n\n", "sites.txt holds no site"),
    ("", "sites.txt holds no site"),
])
def test_sites_file_errors(text, words):
    with pytest.raises(ValueError) as error:
        parse(text)
    assert words in str(error.value)


def test_mask_ends_option():
    from mapdamage_amd import pileup
    assert pileup.parse_mask_ends(None) == (0, 0) and pileup.parse_mask_ends("2") == (2, 2) and pileup.parse_mask_ends("3,0") == (3, 0)
    assert pileup.parse_mask_ends("0") == (0, 0) and pileup.parse_mask_ends("255, 1") == (255, 1)
    for bad in ("256", "1,2,3", "-1", "x", "1,", ""):
        with pytest.raises(ValueError):
            pileup.parse_mask_ends(bad)


# ---------------------------------------------------------------------- the command line
BASE = ["-i", "in.bam", "-r", "ref.fa"]


@pytest.fixture()
def site_files(tmp_path):
    (tmp_path / "plain.txt").write_text("# sites\nchr1\t5\nchr1\t9\n")
    (tmp_path / "alleles.txt").write_text("chr1\t5\tA\tG\trs1\n")
    (tmp_path / "empty.txt").write_text("# none\n")
    return tmp_path


@pytest.mark.parametrize("extra,words", [
    (["--pileup-min-basequal", "20"], "--pileup-min-basequal needs --pileup-sites"),
    (["--pileup-mask-ends", "2"], "--pileup-mask-ends needs --pileup-sites"),
    (["--pileup-call", "majority"], "--pileup-call needs --pileup-sites"),
    (["--pileup-seed", "0"], "--pileup-seed needs --pileup-sites"),
    (["--pileup-min-depth", "1"], "--pileup-min-depth needs --pileup-sites"),
    (["--pileup-single-strand-mode"], "--pileup-single-strand-mode needs --pileup-sites"),
    (["--pileup-seed", "3", "--pileup-call", "none"], "--pileup-call / --pileup-seed need --pileup-sites"),
    (["--pileup-sites", "{plain}", "--pileup-single-strand-mode"], "--pileup-single-strand-mode needs Ref and Alt on every site"),
    (["--pileup-sites", "{plain}", "--host-decode"], "not with --host-decode"),
    (["--pileup-sites", "{plain}", "--gpus", "2"], "--pileup-sites cannot be combined with --gpus 2"),
    (["--pileup-sites", "{plain}", "-n", "1"], "--pileup-sites cannot be combined with -n 1"),
    (["--pileup-sites", "{plain}", "-n", "5000"], "--pileup-sites cannot be combined with -n 5000"),
    (["--pileup-sites", "{plain}", "--rescale-only"], "--pileup-sites belongs to the tabulation pass"),
    (["--pileup-sites", "{plain}", "--stats-only", "--use-raw-nick-freq", "-d", "."], "--pileup-sites belongs to the tabulation pass"),
    (["--pileup-sites", "{plain}", "--pileup-min-basequal", "94"], "--pileup-min-basequal 94: a quality is 0..93"),
    (["--pileup-sites", "{plain}", "--pileup-min-basequal", "-1"], "--pileup-min-basequal -1: a quality is 0..93"),
    (["--pileup-sites", "{plain}", "--pileup-min-basequal", "30", "-Q", "20"], "--pileup-min-basequal 30 is above --min-basequal 20"),
    (["--pileup-sites", "{plain}", "--pileup-mask-ends", "256"], "--pileup-mask-ends: 256 is above 255 bases"),
    (["--pileup-sites", "{plain}", "--pileup-mask-ends", "1,2,3"], "--pileup-mask-ends: '1,2,3' has more than two numbers"),
    (["--pileup-sites", "{plain}", "--pileup-call", "both"], "invalid choice"),
    (["--pileup-sites", "{plain}", "--pileup-seed", "-1"], "--pileup-seed -1"),
    (["--pileup-sites", "{plain}", "--pileup-min-depth", "0"], "--pileup-min-depth 0: at least 1"),
    (["--pileup-sites", "{none}"], "No such file"),
    (["--pileup-sites", "{empty}"], "holds no site"),
])
def test_argument_errors(capsys, site_files, extra, words):
    from mapdamage_amd.main import parse_args
    files = dict(plain=site_files / "plain.txt", alleles=site_files / "alleles.txt", empty=site_files / "empty.txt", none=site_files / "none.txt")
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + [e.format(**files) for e in extra])
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_arguments_that_pass(site_files, tmp_path):
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "plain.txt")])
    assert (o.pileup_min_basequal, o.pileup_mask_ends, o.pileup_call, o.pileup_seed, o.pileup_min_depth, o.pileup_single_strand_mode) == (0, (0, 0), "random", 0, 1, False)
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "alleles.txt"), "--pileup-min-basequal", "30", "--pileup-mask-ends", "2,3", "--pileup-call", "majority",
                           "--pileup-seed", str(2**64 - 1), "--pileup-min-depth", "3", "--pileup-single-strand-mode", "--depth", "--remove-duplicates", "-n", "0.5",
                           "--by-pmd-score", "--merge-libraries", "--min-mapq", "25", "--write-kept", str(tmp_path / "k.bam"), "--mask-ends", "2,2", "--chunk-mb", "1"])
    assert (o.pileup_min_basequal, o.pileup_mask_ends, o.pileup_call, o.pileup_seed, o.pileup_min_depth, o.pileup_single_strand_mode) == (30, (2, 3), "majority", 2**64 - 1, 3, True)
    o = parse_args(BASE + ["--pileup-sites", str(site_files / "plain.txt"), "--pileup-min-basequal", "20", "-Q", "20"])
    assert o.pileup_min_basequal == 20 and o.minqual == 20
    o = parse_args(BASE)
    assert o.pileup_sites is None and o.pileup_call is None and not o.pileup_single_strand_mode


# ---------------------------------------------------------------------- the emitters
def test_emitters(tmp_path, monkeypatch):
    from mapdamage_amd import pileup
    sites = parse("chrM\t3\tC\tT\trs2\nchr1\t10\tA\tG\trs1\nscaf/1:a\t7\tG\tC\n")
    counters = np.array([[1, 0, 2, 0, 0, 0, 1, 0, 1, 2, 3, 4], [0] * 12, [0, 0, 0, 2**32 - 1, 0, 0, 0, 1, 0, 0, 0, 9]], np.uint32)
    refbase, call, depth = np.array([b"A", b"N", b"T"], "S1"), np.array([b"G", b"N", b"T"], "S1"), np.array([4, 0, 2**32 - 1], np.uint32)
    counters[2, 7] = 0
    head = "Sequence\tPosition\tId\tRef\tAlt\tRefBase\tA+\tC+\tG+\tT+\tA-\tC-\tG-\tT-\tDeletions\tLowQual\tOther\tMasked\tDepth"
    want = (head + "\tCall\nchr1\t10\trs1\tA\tG\tA\t1\t0\t2\t0\t0\t0\t1\t0\t1\t2\t3\t4\t4\tG\n"
            "chrM\t3\trs2\tC\tT\tN\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tN\n"
            "scaf/1:a\t7\t.\tG\tC\tT\t0\t0\t0\t4294967295\t0\t0\t0\t0\t0\t0\t0\t9\t4294967295\tT\n")
    text = b"".join(pileup.pileup_chunks(NAMES, sites, counters, refbase, call, depth)).decode()
    site_list = list(zip(sites.tid.tolist(), sites.pos.tolist()))
    assert text == want == PR.pileup_text(NAMES, site_list, sites.ids, ["AG", "CT", "GC"], "ANT", counters, "GNT")
    assert b"".join(pileup.pileup_chunks(NAMES, sites, counters, refbase, call, depth, chunk=2)).decode() == want
    # without alleles and without the Call column
    plain = parse("chrM\t3\nchr1\t10\nscaf/1:a\t7\n")
    text = b"".join(pileup.pileup_chunks(NAMES, plain, counters, refbase, call, depth, with_call=False)).decode()
    assert text == PR.pileup_text(NAMES, site_list, None, None, "ANT", counters, None)
    assert text.splitlines()[0] == head and text.splitlines()[1] == "chr1\t10\t.\t.\t.\tA\t1\t0\t2\t0\t0\t0\t1\t0\t1\t2\t3\t4\t4"
    pileup.write_pileup(tmp_path / "pileup.tsv", NAMES, sites, counters, refbase, call, depth)
    assert (tmp_path / "pileup.tsv").read_text() == want and os.listdir(tmp_path) == ["pileup.tsv"]
    # the summary and the log line
    counts = dict(counted=11, outside=2, over_a_site=5, pairs=7)
    values = dict(path="panel.txt", min_basequal=20, mask_ends=(2, 3), call="majority", seed=5, min_depth=1, single_strand=True)
    summary = pileup.summary_text(values, counters, call, depth, counts)
    assert summary == ("SitesFile\tMinBaseQual\tMaskEnds\tCall\tSeed\tMinDepth\tSingleStrandMode\tSites\tCovered\tCalled\tSumDepth\tMeanDepth\tRecordsCounted\t"
                       "RecordsOutside\tRecordsOverASite\tPairs\tDeletions\tLowQual\tOther\tMasked\n"
                       "panel.txt\t20\t2,3\tmajority\t5\t1\t1\t3\t2\t2\t4294967299\t1431655766.33333\t11\t2\t5\t7\t1\t2\t3\t13\n")
    assert summary == PR.summary_text("panel.txt", 20, 2, 3, "majority", 5, 1, True, counters, "GNT", counts)
    line = pileup.log_line(values, counters, call, depth, counts)
    assert line == ("Pileup: 3 sites, 2 covered (66.67 %), 2 called (majority, seed 5), mean depth 1.43166e+09 at sites; 5 of 11 records over a site; "
                    "2 records outside their sequence") == PR.log_line("majority", 5, counters, "GNT", counts)
    values["call"] = "none"
    assert "0 called (none)" in pileup.log_line(values, counters, call, depth, counts) == PR.log_line("none", 5, counters, None, counts)
    assert pileup.summary_text(values, counters, call, depth, counts) == PR.summary_text("panel.txt", 20, 2, 3, "none", 5, 1, True, counters, None, counts)
    # the reference's letter that is neither allele
    assert pileup.off_build(sites, refbase) == 2 and pileup.off_build(plain, refbase) == 0         # (N at C/T, T at G/C)
    assert pileup.off_build(sites, np.array([b"G", b"C", b"T"], "S1")) == 1
    # a failure on the way removes the temporary file and leaves an earlier file alone
    def broken(*args, **kwargs):
        yield b"Sequence\n"
        raise OSError("disk full")
    monkeypatch.setattr(pileup, "pileup_chunks", broken)
    with pytest.raises(OSError):
        pileup.write_pileup(tmp_path / "pileup.tsv", NAMES, sites, counters, refbase, call, depth)
    assert os.listdir(tmp_path) == ["pileup.tsv"] and (tmp_path / "pileup.tsv").read_text() == want
