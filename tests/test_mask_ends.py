"""--mask-ends without a GPU: the rule header (csrc/mdx_kept_mask.h) built for the host against its restatement
(tests/mask_rule.py) on crafted records and a random pool, the same records through a program of its own under the
sanitizers, and the command line's options and argument errors."""

import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mask_rule as M
from tests.test_write_kept import error_of, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
KS = ((1, 0), (0, 1), (2, 2), (3, 1), (255, 255))
PARAMS = [(k5, k3, what, ss) for what in M.MODES for ss in (0, 1) for k5, k3 in KS]


# ---------------------------------------------------------------------- the reference, the records
@functools.lru_cache(maxsize=None)
def genome():
    """Three sequences: 300 bases — the first 64 of them C and G only, so that every aligned base there has a partner above it,
    N at 100 to 102 —, 60 bases, 5 bases."""
    rng = np.random.default_rng(5)
    g0 = "".join(rng.choice(list("CG"), 64)) + "".join(rng.choice(list("ACGT"), 236))
    g0 = g0[:100] + "NNN" + g0[103:]
    return [g0, "".join(rng.choice(list("ACGT"), 60)), "GCCGA"]


def device_reference(ref):
    """(bases, contig_off) as the context keeps them: ASCII for A C G T, a byte above 0x7F for the rest."""
    bases = np.frombuffer("".join(ref).encode(), np.uint8).copy()
    bases[~np.isin(bases, np.frombuffer(b"ACGT", np.uint8))] = 0x85
    return bases, np.concatenate([[0], np.cumsum([len(s) for s in ref])]).astype(np.int64)


def from_ref(cigar, tid, pos, plant, rng=None):
    """A SEQ for the CIGAR over the reference: an aligned base is the reference's, or — where ``plant(q, n_query)`` says so —
    T above C and A above G; T above what is no base; inserted and clipped bases alternate T and A."""
    ref = genome()[tid] if 0 <= tid < len(genome()) else ""
    ops = M.parse_cigar(cigar) if isinstance(cigar, str) else cigar
    n_query = sum(n for op, n in ops if op in "MIS=X")
    seq, r = [], pos
    for op, n in ops:
        for _ in range(n):
            if op in "M=X":
                base = ref[r] if 0 <= r < len(ref) else "A"
                if base not in "ACGT":
                    base = "T"
                elif plant(len(seq), n_query):
                    base = {"C": "T", "G": "A"}.get(base, base)
                elif rng is not None and rng.random() < 0.05:
                    base = "ACGT"[rng.integers(4)]
                seq.append(base)
                r += 1
            elif op in "IS":
                seq.append("TA"[len(seq) % 2])
            elif op in "DN":
                r += 1
    return "".join(seq)


def every_other(q, n):
    return q % 2 == 0


@functools.lru_cache(maxsize=None)
def crafted():
    """(label, body) of the records of the issue's list, each on both strands."""
    out = []

    def add(label, cigar, seq=None, tid=0, pos=0, cut=None, **kw):
        for flag in (0, 0x10):
            s = from_ref(cigar, tid, pos, every_other) if seq is None else seq
            body = M.make_record(cigar, s, flag=flag | 0x1, tid=tid, pos=pos, tags=b"NMC\x01MDZ5\0", **kw)
            out.append(("%s %s" % (label, "-" if flag else "+"), body if cut is None else body[:cut(body)]))

    for n in range(1, 6):                                   # odd and even, the padding nibble
        add("l_seq %d" % n, "%dM" % n, pad=0xA)
        add("l_seq %d at 1" % n, "%dM" % n, pos=1, pad=0x5, qual=list(range(1, n + 1)))
    for cigar in ("2S6M", "6M2S", "2S6M3S", "1H2S6M", "6M2S1H", "2H2S6M2S3H", "7S1M", "1M7S", "3S1M4S", "8S", "2H3S", "3S2H", "1H8M1H"):
        add("clips " + cigar, cigar, pos=3)
    add("no bases", "", "")
    add("no bases, a CIGAR", "5M", "")
    add("no CIGAR", "", "TACGTTA")
    add("no CIGAR, one base", "", "T")
    add("CIGAR too short", "5M", "TACGTA")
    add("CIGAR too long", "3S5M", "TACGTA")
    add("cut in QUAL", "6M", cut=lambda b: M.decode(b)["qual_at"] + 5)
    add("cut in SEQ", "6M", cut=lambda b: M.decode(b)["seq_at"] + 1)
    add("cut in the CIGAR", "6M", cut=lambda b: 35)
    add("cut in the header", "6M", cut=lambda b: 31)
    add("nothing", "6M", cut=lambda b: 0)
    add("whole to the byte", "6M", cut=lambda b: M.decode(b)["qual_at"] + 6)
    add("no qualities", "6M", qual=[0xFF] * 6)
    add("first quality 0xFF", "6M", qual=[0xFF, 30, 31, 32, 33, 34])
    add("last quality 0xFF", "6M", qual=[30, 31, 32, 33, 34, 0xFF])
    for cigar in ("2I6M", "6M2I", "1S2I6M", "6M2I1S", "3M2I3M", "1M1I1M1I1M", "1I"):
        add("insertion " + cigar, cigar, pos=2)
    for cigar in ("1M2D5M", "1M3N5M", "5M2D1M", "5M3N1M", "1M1D1M1N1M1D1M", "2D4M", "4M2N"):
        add("gap " + cigar, cigar, pos=5)
    for cigar in ("2=1X3=", "1X5=1X", "1=", "1X"):
        add("match operations " + cigar, cigar, pos=7)
    add("padding operation", "2M1P4M")
    add("nibbles = and IUPAC", "7M", "=TRYNA=")
    add("N there already", "5M", "NNTAN")
    add("IUPAC at the ends", "6M", "WTCGAK")
    add("refID -1", "6M", tid=-1)
    add("refID -1, T and A", "6M", "TTCGAA", tid=-1, pos=-1)
    add("refID 3", "6M", "TTCGAA", tid=3)
    add("pos -1", "6M", "TTCGAA", pos=-1)
    add("ends at the end", "6M", tid=1, pos=54)
    add("ends one past the end", "6M", tid=1, pos=55)
    add("ends at the end, a deletion", "3M2D3M", tid=1, pos=52)
    add("ends one past the end, a deletion", "3M2D3M", tid=1, pos=53)
    add("the whole of a sequence", "5M", tid=2)
    add("longer than its sequence", "6M", tid=2)
    add("no base in the reference", "6M", pos=98)
    add("no base in the reference, first", "4M", pos=100)
    add("no base in the reference, last", "4M", pos=99)
    add("long, both windows whole", "300M", "".join("TACG"[i % 4] for i in range(300)))
    return out


@functools.lru_cache(maxsize=None)
def pool(n=3000):
    """Random records over the genome: 1 to 40 bases, CIGARs of M I D N S H = X, C>T and G>A planted at both ends; one in
    twelve is one the rule leaves alone or finds no reference for."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(n):
        l_seq = int(rng.integers(1, 41))
        left = min(int(rng.integers(0, 4)) if rng.random() < 0.3 else 0, l_seq - 1)
        right = min(int(rng.integers(0, 4)) if rng.random() < 0.3 else 0, l_seq - 1 - left)
        core, ops = l_seq - left - right, []
        while core > 0:
            step = int(rng.integers(1, core + 1))
            ops.append(("M=X"[int(rng.choice(3, p=(0.8, 0.1, 0.1)))], step))
            core -= step
            if core > 0:
                gap = "IDN-"[int(rng.choice(4, p=(0.3, 0.3, 0.1, 0.3)))]
                if gap == "I":
                    step = int(rng.integers(1, core + 1)) if core > 1 else 0
                    if step and core - step > 0:
                        ops.append(("I", step))
                        core -= step
                elif gap in "DN":
                    ops.append((gap, int(rng.integers(1, 4))))
        if rng.random() < 0.1:                      # an insertion at an end of the query
            first = ops[0]
            if first[0] == "M" and first[1] > 1:
                ops[0:1] = [("I", 1), ("M", first[1] - 1)] if rng.random() < 0.5 else ops[0:1]
            last = ops[-1]
            if last[0] == "M" and last[1] > 1 and rng.random() < 0.5:
                ops[-1:] = [("M", last[1] - 1), ("I", 1)]
        ops = ([("S", left)] if left else []) + ops + ([("S", right)] if right else [])
        if rng.random() < 0.15:
            ops = [("H", 2)] + ops
        if rng.random() < 0.15:
            ops = ops + [("H", 3)]
        span = sum(k for op, k in ops if op in "MDN=X")
        tid = int(rng.choice(2, p=(0.7, 0.3))) if span <= len(genome()[1]) else 0
        pos = int(rng.integers(0, len(genome()[tid]) - span + 1))
        flag = 0x10 if rng.random() < 0.5 else 0
        seq = from_ref(ops, tid, pos, lambda q, nq: (q < left + 4 or q >= nq - right - 4) and rng.random() < 0.7, rng)
        qual = [int(x) for x in rng.integers(2, 42, l_seq)]
        broken = int(rng.integers(0, 72))
        kw = {}
        if broken == 0:
            tid = -1
        elif broken == 1:
            tid = 3
        elif broken == 2:
            pos = len(genome()[tid]) - span + 1 + int(rng.integers(0, 3))
        elif broken == 3:
            ops = ops + [("M", 1)]
        elif broken == 4:
            ops = []
        elif broken == 5:
            qual = [0xFF] * l_seq
        body = M.make_record(ops, seq, qual, flag=flag, tid=tid, pos=pos, name=b"p%d" % i, tags=b"NMC\x02" if i % 3 else b"", pad=i % 16, **kw)
        if broken == 6:
            body = body[:len(body) - (4 if i % 3 else 0) - 1 - int(rng.integers(0, l_seq))]
        out.append(body)
    return out


# ---------------------------------------------------------------------- the host build of the rule
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("mask") / "mask_ends_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "mask_ends_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.kept_mask_valid_host.argtypes = [ctypes.c_int64] * 4
    return lib


def host_rule(lib, bodies, k5, k3, what, ss, ref=None):
    """[(record masked, count)] by the header's lines."""
    bases, contig_off = device_reference(genome() if ref is None else ref)
    # every record in a buffer of its own bytes, 0xEE between them: a store outside a record shows
    gap, off, at = 8, [], 8
    for b in bodies:
        off.append(at)
        at += len(b) + gap
    data = np.full(at, 0xEE, np.uint8)
    for o, b in zip(off, bodies):
        data[o:o + len(b)] = np.frombuffer(b, np.uint8)
    off, bs = np.asarray(off, np.uint64), np.asarray([len(b) for b in bodies], np.uint32)
    counts = np.zeros(len(bodies), np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.kept_mask_records_host(ctypes.c_int64(len(bodies)), p(data), p(off), p(bs), ctypes.c_uint32(k5), ctypes.c_uint32(k3),
                               ctypes.c_uint32(M.MODES.index(what)), ctypes.c_uint32(ss), p(bases), p(contig_off),
                               ctypes.c_int32(len(contig_off) - 1), p(counts))
    out = []
    for o, b, c in zip(off.tolist(), bodies, counts.tolist()):
        assert (data[o - gap:o] == 0xEE).all() and (data[o + len(b):o + len(b) + gap] == 0xEE).all()
        out.append((data[o:o + len(b)].tobytes(), c))
    return out


def test_modes_are_the_headers(host):
    import re
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    for i, name in enumerate(("ALL", "TRANSITIONS", "MISMATCHES")):
        assert host.kept_mask_mode_host(i) == i == int(re.search(r"#define MDX_MASK_%s (\d+)" % name, text).group(1))
    from mapdamage_amd.sam import MASK_WHAT
    assert tuple(MASK_WHAT) == M.MODES


def test_valid_parameters(host):
    for k5, k3, what, ss, ok in [(1, 0, 0, 0, 1), (0, 1, 2, 1, 1), (255, 255, 1, 0, 1), (0, 0, 0, 0, 0), (256, 1, 0, 0, 0), (1, 256, 0, 0, 0),
                                 (-1, 1, 0, 0, 0), (1, -1, 0, 0, 0), (1, 1, 3, 0, 0), (1, 1, -1, 0, 0), (1, 1, 0, 2, 0), (1, 1, 0, -1, 0),
                                 (1 << 32, 1, 0, 0, 0), (1, 1, 1 << 32, 0, 0)]:
        assert host.kept_mask_valid_host(k5, k3, what, ss) == ok, (k5, k3, what, ss)


def outside_unchanged(before, after):
    rec = M.decode(before)
    if rec is None:
        return before == after
    return len(before) == len(after) and before[:rec["seq_at"]] == after[:rec["seq_at"]] and \
        before[rec["qual_at"] + rec["l_seq"]:] == after[rec["qual_at"] + rec["l_seq"]:]


@pytest.mark.parametrize("what", M.MODES)
def test_crafted_records(host, what):
    labels, bodies = [c[0] for c in crafted()], [c[1] for c in crafted()]
    selected_somewhere = set()
    for k5, k3, mode, ss in PARAMS:
        if mode != what:
            continue
        got = host_rule(host, bodies, k5, k3, what, ss)
        for label, body, (masked, count) in zip(labels, bodies, got):
            want = M.apply(body, k5, k3, what, bool(ss), genome())
            assert (masked, count) == want, (label, k5, k3, what, ss)
            assert outside_unchanged(body, masked), label
            if count:
                selected_somewhere.add(label)
    # the cases that must leave the record alone do, and the others are not idle (the restatement's word)
    idle = {label for label in labels if label not in selected_somewhere}
    always_idle = ("no bases", "CIGAR too", "cut in", "nothing", "clips 8S", "clips 2H3S", "clips 3S2H")
    assert what != M.ALL or all(label.startswith(always_idle) for label in idle), sorted(idle)
    for label in labels:
        if label.startswith(always_idle):
            assert label in idle
        if what == M.MISMATCHES and label.startswith(("no CIGAR", "refID", "pos -1", "ends one past", "longer than")):
            assert label in idle, label
    for label in ("l_seq 1 +", "l_seq 5 -", "clips 2H2S6M2S3H +", "gap 1M2D5M -", "ends at the end -", "the whole of a sequence +"):
        assert label in selected_somewhere, label


def test_crafted_details():
    """A few of the restatement's answers by hand, so that the yardstick is not only compared with itself."""
    body = M.make_record("2S4M1S", "TTTCATA", [10, 11, 12, 13, 14, 15, 16], pad=0x9)
    masked, count = M.apply(body, 1, 2, M.ALL)
    rec = M.decode(masked)
    assert count == 3 and "".join(M.NIBBLES[x] for x in rec["nibbles"]) == "TTNCNNAW"
    assert rec["qual"] == [10, 11, 0, 13, 0, 0, 16]
    rev = M.make_record("2S4M1S", "TTTCATA", [10, 11, 12, 13, 14, 15, 16], flag=0x10)
    rec = M.decode(M.apply(rev, 1, 2, M.ALL)[0])
    assert rec["qual"] == [10, 11, 0, 0, 14, 0, 16]
    # transitions: forward 5' T, 3' A; reverse 5' (right) A, 3' (left) T; single-stranded 3' as 5'
    fwd = M.make_record("4M", "TAAT")
    assert [M.apply(fwd, 4, 0, M.TRANSITIONS)[1], M.apply(fwd, 0, 1, M.TRANSITIONS)[1], M.apply(fwd, 0, 1, M.TRANSITIONS, True)[1]] == [2, 0, 1]
    rev = M.make_record("4M", "TAAT", flag=0x10)
    assert M.decode(M.apply(rev, 2, 0, M.TRANSITIONS)[0])["nibbles"][:4] == [8, 1, 15, 8]
    assert M.decode(M.apply(rev, 0, 2, M.TRANSITIONS)[0])["nibbles"][:4] == [15, 1, 1, 8]
    assert M.decode(M.apply(rev, 0, 2, M.TRANSITIONS, True)[0])["nibbles"][:4] == [8, 15, 1, 8]
    # mismatches: the reference under the base, behind a deletion
    ref = ["ACCGGT"]
    rec = M.make_record("1M2D2M", "ATT", pos=0)          # A over A, T over G, T over G
    assert M.apply(rec, 3, 0, M.MISMATCHES, False, ref)[1] == 0
    rec = M.make_record("1M1D2M", "ATT", pos=0)          # A over A, T over C, T over G
    masked, count = M.apply(rec, 3, 0, M.MISMATCHES, False, ref)
    assert count == 1 and M.decode(masked)["nibbles"][:3] == [1, 15, 8]
    assert M.apply(M.make_record("3M", "ATT", pos=4), 3, 0, M.ALL, False, ref)[1] == 3
    assert M.apply(M.make_record("3M", "ATT", pos=4), 3, 0, M.MISMATCHES, False, ref)[1] == 0   # beyond the sequence


def test_random_pool(host):
    bodies = pool()
    untouched = {what: 0 for what in M.MODES}
    reached = {}
    for k5, k3, what, ss in PARAMS:
        got = host_rule(host, bodies, k5, k3, what, ss)
        alone = 0
        for i, (body, (masked, count)) in enumerate(zip(bodies, got)):
            want = M.apply(body, k5, k3, what, bool(ss), genome())
            assert (masked, count) == want, (i, k5, k3, what, ss)
            assert outside_unchanged(body, masked), i
            assert (count == 0) == (masked == body) or what == M.ALL        # (ALL counts an N that was there already)
            alone += count == 0
            if count and (k5 == 0 or k3 == 0) and ss == 0:
                key = (what, bool(struct.unpack_from("<H", body, 14)[0] & 0x10), "5p" if k3 == 0 else "3p")
                reached[key] = reached.get(key, 0) + 1
        if (k5, k3) == (255, 255):
            untouched[what] = alone
    # on the restatement's output: every mode, strand and end has work, every mode leaves records alone (even at 255, 255)
    for what in M.MODES:
        for reverse in (False, True):
            for end in ("5p", "3p"):
                assert reached.get((what, reverse, end), 0) >= 20, (what, reverse, end, reached)
        assert untouched[what] >= 20, untouched


def test_under_the_sanitizers(tmp_path):
    """The crafted records and a part of the pool through a program of its own built with -fsanitize=address,undefined:
    every record in a heap block of exactly its bytes, the reference in one of exactly its length."""
    exe = tmp_path / "mask_walk"
    subprocess.check_call(["c++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "mask_ends_walk_main.cpp"), "-o", str(exe)])
    bases, contig_off = device_reference(genome())
    bodies = [c[1] for c in crafted()] + pool()[:400]
    n_cases = 0
    with open(tmp_path / "cases.bin", "wb") as out:
        out.write(struct.pack("<i", len(contig_off) - 1) + contig_off.tobytes() + bases.tobytes())
        for k5, k3, what, ss in PARAMS:
            for body in bodies:
                masked, count = M.apply(body, k5, k3, what, bool(ss), genome())
                out.write(struct.pack("<BBBBII", k5, k3, M.MODES.index(what), ss, count, len(body)) + body + masked)
                n_cases += 1
    done = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, timeout=300)
    assert done.returncode == 0, done.stdout.decode()[-2000:] + done.stderr.decode()[-4000:]
    assert done.stdout.decode().splitlines()[-1] == "%d cases masked, 0 wrong" % n_cases and not done.stderr


# ---------------------------------------------------------------------- the command line
def test_options(tmp_path):
    out = tmp_path / "kept.bam"
    o = parse(tmp_path, "--write-kept", out, "--mask-ends", "2")
    assert (o.mask_ends, o.mask_what, o.single_stranded) == ((2, 2), "all", False)
    o = parse(tmp_path, "--write-kept", out, "--mask-ends", "2,1", "--mask-what", "mismatches", "--single-stranded")
    assert (o.mask_ends, o.mask_what, o.single_stranded) == ((2, 1), "mismatches", True)
    assert parse(tmp_path, "--write-kept", out, "--mask-ends", "0,255", "--mask-what", "transitions").mask_ends == (0, 255)
    assert parse(tmp_path, "--write-kept", out, "--mask-ends", " 3 , 0 ").mask_ends == (3, 0)
    for args in ([], ["--write-kept", out]):
        o = parse(tmp_path, *args)
        assert o.mask_ends is None and o.mask_what is None


@pytest.mark.parametrize("extra", [
    ["--by-pmd-score", "--write-groups", "1", "--tag-group", "XG", "--tag-pmd-score", "DS", "--write-index"],
    ["--by-reference", "--min-mapq", "25", "--exclude-flags", "0x400", "-n", "0.5", "--downsample-seed", "7"],
    ["-Q", "20", "--regions", "panel.bed", "--only-regions", "--chunk-mb", "64"],
])
def test_allowed_combinations(tmp_path, extra):
    o = parse(tmp_path, "--write-kept", tmp_path / "kept.bam", "--mask-ends", "2,2", *extra)
    assert o.mask_ends == (2, 2)


def test_allowed_with_the_estimate_and_rescale(tmp_path):
    from mapdamage_amd.main import parse_args
    o = parse_args(["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out"), "--write-kept", str(tmp_path / "kept.bam"), "--stats",
                    "--rescale", "--single-stranded", "--mask-ends", "3,1", "--mask-what", "transitions"])
    assert o.want_stats and o.rescale and (o.mask_ends, o.mask_what) == ((3, 1), "transitions")


def test_argument_errors(tmp_path, capsys):
    out = tmp_path / "kept.bam"
    assert "--mask-ends needs --write-kept" in error_of(tmp_path, capsys, "--mask-ends", "2")
    assert "--mask-what needs --mask-ends" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-what", "all")
    assert "--mask-what needs --mask-ends" in error_of(tmp_path, capsys, "--mask-what", "transitions")
    assert "invalid choice" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "2", "--mask-what", "everything")
    assert "--mask-ends: both ends are 0 bases" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "0")
    assert "--mask-ends: both ends are 0 bases" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "0,0")
    assert "--mask-ends: 256 is above 255 bases" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "256")
    assert "--mask-ends: 300 is above 255 bases" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "1,300")
    for bad in ("-1", "2,", ",2", "a", "1.5", "2;2", ""):
        assert "is not a number of bases" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends=" + bad), bad
    assert "has more than two numbers" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "1,2,3")
    # the restrictions of --write-kept stand as they are
    assert "--write-kept is written by the device decode path: not with --host-decode" in error_of(
        tmp_path, capsys, "--write-kept", out, "--mask-ends", "2", "--host-decode")
    assert "--write-kept cannot be combined with --gpus 2" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "2", "--gpus", "2")
    assert "--write-kept cannot be combined with -n 1000" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "2", "-n", "1000")
    assert "--write-kept belongs to the tabulation pass" in error_of(tmp_path, capsys, "--write-kept", out, "--mask-ends", "2", "--rescale-only")
