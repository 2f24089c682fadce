"""--calmd without a GPU: the rule header (csrc/mdx_kept_md.h) built for the host against its restatement (tests/md_rule.py)
and the restatement's inverse on the issue's ten hand-derived cases, crafted records and a random pool, the same records
through a program of its own under the sanitizers, and the command line's option and argument errors."""

import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mask_rule as M
from tests import md_rule as R
from tests.test_mask_ends import crafted as mask_crafted
from tests.test_mask_ends import device_reference, from_ref, genome, pool
from tests.test_write_kept import error_of, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")

# the issue's table: reference, CIGAR, read (None: the reference's own bases), MD, NM
LITERAL = [
    ("ACGTACGTAC", "10M", None, "10", 0),
    ("ACGTACGTAC", "4M2D4M", "ACGTGTAC", "4^AC4", 2),
    ("ACGTAC", "3M1I3M", "ACGTTAC", "6", 1),
    ("ACGTA", "5M", "TCGTC", "0A3A0", 2),
    ("ACGTA", "2M1D2M", "ACCA", "2^G0T1", 2),
    ("ACGTACG", "2M3N2M", "ACCG", "4", 0),
    ("ACG", "2S3M", "TTACG", "3", 0),
    ("ACGT", "4M", "ANGT", "1C2", 1),
    ("ANGT", "4M", "ACGT", "1N2", 1),
    ("ACGT", "4M", "====", "4", 0),
]


def never(q, n):
    return False


def other_base(base):
    return {"A": "C", "C": "A", "G": "T", "T": "G"}.get(base, "A")


@functools.lru_cache(maxsize=None)
def crafted():
    """(label, body, recomputed?) of the records of the issue's list, over the genome of tests/test_mask_ends.py."""
    out = []
    g0 = genome()[0]

    def add(label, cigar, done=True, seq=None, tid=0, pos=0, cut=None, tags=b"", **kw):
        s = from_ref(cigar, tid, pos, never) if seq is None else seq
        body = M.make_record(cigar, s, tid=tid, pos=pos, tags=tags, **kw)
        out.append((label, body if cut is None else body[:cut(body)], done))

    nm, md, long_md = b"NMC\x09", b"MDZ7A7\0", b"MDZ" + b"1A" * 100 + b"1\0"
    xa, xb, xz = b"XAi\x01\x02\x03\x04", b"XBBs\x03\x00\x00\x00\x01\x00\x02\x00\x03\x00", b"XZZhello\0"
    # where the old fields stand
    add("tags first", "8M", tags=nm + md + xa + xz, pos=4)
    add("tags in the middle", "8M", tags=xa + nm + xz + md + xb, pos=4)
    add("tags last", "8M", tags=xa + xz + nm + md, pos=4)
    add("tags twice", "8M", tags=nm + xa + md + xz + nm + xb + md + xa, pos=4)
    add("NM three times running", "8M", tags=nm + nm + nm + xa, pos=4)
    add("other types", "8M", tags=b"NMi\x01\x00\x00\x00" + xa + b"MDAx", pos=4)
    add("NM as a string", "8M", tags=b"NMZnine\0" + xa, pos=4)
    add("behind a B array", "8M", tags=xb + nm + md, pos=4)
    add("behind an empty B array", "8M", tags=b"XBBC\x00\x00\x00\x00" + md, pos=4)
    add("an old MD longer than the new one", "8M", tags=xa + long_md + nm, pos=4)
    add("only an old MD", "8M", tags=long_md, pos=4)
    add("no tags at all", "8M", pos=4)
    add("other tags only", "8M", tags=xa + xb + xz, pos=4)
    add("reverse strand", "3S5M2D4M", tags=nm + md, pos=9, flag=0x10)
    add("reverse strand, mismatches", "9M", seq="".join(other_base(c) if i % 3 == 0 else c for i, c in enumerate(g0[20:29])), pos=20, flag=0x10)
    # the walk
    add("every base a mismatch", "7M", seq="".join(other_base(c) for c in g0[30:37]), pos=30, tags=nm)
    add("odd length, one base", "1M", pos=11)
    add("no base in the reference", "6M", pos=98)
    add("N above no base", "4M", pos=99, seq="ANNA")
    add("IUPAC and = in the read", "7M", seq="=" + g0[41] + "R" + g0[43] + "N" + g0[45] + "=", pos=40)
    add("match operations", "2=1X3=", pos=7, tags=md)
    add("a deletion first", "2D4M", pos=5)
    add("a deletion behind a mismatch", "1M1D3M", seq=other_base(g0[50]) + from_ref("3M", 0, 52, never), pos=50)
    add("gaps of both kinds", "1M1D1M1N1M1D1M", pos=5, tags=nm + md)
    add("insertions", "1I3M2I3M1I", pos=2, tags=md)
    add("clips and a padding", "1H2S2M1P4M2S1H", pos=3, tags=nm)
    add("the whole of a sequence", "5M", tid=2)
    add("ends at the end, a deletion", "3M2D3M", tid=1, pos=52)
    add("a run of ten and of a hundred", "120M", seq="".join(other_base(c) if i in (10, 111) else c for i, c in enumerate(g0[150:270])), pos=150)
    # NM's three types (an insertion of that many bases between two matching ones)
    for n in (255, 256, 65535, 65536):
        add("NM %d" % n, "1M%dI1M" % n, pos=60, tags=nm)
    # the cap: two mismatches around a deletion of d bases give 7 + d characters; 2 * 2 + 64 = 68
    for d, done in ((61, True), (62, False)):
        add("cap %s" % ("met" if done else "passed"), "1M%dD1M" % d, done, seq=other_base(g0[70]) + other_base(g0[70 + d + 1]), pos=70, tags=nm + md)
    # each reason to skip
    add("skip: cut in the header", "6M", False, cut=lambda b: 31, tags=nm)
    add("skip: nothing", "6M", False, cut=lambda b: 0)
    add("skip: no bases", "", False, seq="", tags=nm + md)
    add("skip: no CIGAR", "", False, seq="TACGTTA", tags=nm + md)
    add("skip: cut in QUAL", "6M", False, cut=lambda b: M.decode(b)["qual_at"] + 5)
    add("skip: CIGAR too short", "5M", False, seq="TACGTA", tags=nm + md)
    add("skip: CIGAR too long", "3S5M", False, seq="TACGTA", tags=md)
    add("skip: refID -1", "6M", False, tid=-1, tags=nm)
    add("skip: refID 3", "6M", False, seq="ACGTAC", tid=3, tags=nm)
    add("skip: pos -1", "6M", False, seq="ACGTAC", pos=-1, tags=nm + md)
    add("skip: ends one past the end", "6M", False, tid=1, pos=55, tags=md)
    add("skip: ends one past the end, a deletion", "3M2D3M", False, tid=1, pos=53)
    add("skip: a skip past the end", "3M300N3M", False, pos=10, tags=nm)
    add("skip: an unknown type", "6M", False, tags=xa + b"XQq\x01" + nm)
    add("skip: an unknown type, three bytes at the end", "6M", False, tags=nm + b"XQq")
    add("skip: a B array past the end", "6M", False, tags=nm + b"XBBi\x09\x00\x00\x00\x01\x00\x00\x00")
    add("skip: a B array cut in its count", "6M", False, tags=md + b"XBBi\x09\x00")
    add("skip: a string without its NUL", "6M", False, tags=nm + b"XZZhello")
    add("skip: a field cut off", "6M", False, tags=md + b"XAi\x01\x02")
    add("skip: two bytes behind the tags", "6M", False, tags=nm + b"XA")
    add("skip: CG of type B", "6M", False, tags=nm + b"CGBI\x01\x00\x00\x00\x60\x00\x00\x00" + md)
    add("CG of another type", "6M", tags=nm + b"CGZ6M\0" + md)
    return out


def all_records():
    """The crafted records, those of tests/test_mask_ends.py (NM and MD first, every oddity of SEQ and CIGAR) and its pool."""
    return [c[1] for c in crafted()] + [c[1] for c in mask_crafted()] + pool()


# ---------------------------------------------------------------------- the host build of the rule
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("calmd") / "calmd_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "calmd_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.kept_md_growth_host.argtypes, lib.kept_md_growth_host.restype = [ctypes.c_uint64], ctypes.c_uint64
    return lib


def host_rule(lib, bodies, ref, room):
    """[(record recomputed, recomputed?, had?)] by the header's lines; record i is written into ``room[i]`` bytes with 0xEE
    around them: a store outside shows."""
    bases, contig_off = device_reference(ref)
    gap, off, at = 8, [], 8
    for b in bodies:
        off.append(at)
        at += len(b) + gap
    data = np.full(at, 0xEE, np.uint8)
    for o, b in zip(off, bodies):
        data[o:o + len(b)] = np.frombuffer(b, np.uint8)
    gap, out_off, at = 64, [], 64
    for r in room:
        out_off.append(at)
        at += r + gap
    out = np.full(at, 0xEE, np.uint8)
    off, bs, out_off = np.asarray(off, np.uint64), np.asarray([len(b) for b in bodies], np.uint32), np.asarray(out_off, np.uint64)
    new_bs, flags = np.zeros(len(bodies), np.uint32), np.zeros(len(bodies), np.uint8)
    before = data.copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.kept_md_records_host(ctypes.c_int64(len(bodies)), p(data), p(off), p(bs), p(bases), p(contig_off), ctypes.c_int32(len(contig_off) - 1),
                             p(out), p(out_off), p(new_bs), p(flags))
    assert (data == before).all()
    got = []
    for o, r, n, fl in zip(out_off.tolist(), room, new_bs.tolist(), flags.tolist()):
        assert n <= r and (out[o - gap:o] == 0xEE).all() and (out[o + r:o + r + gap] == 0xEE).all() and (out[o + n:o + r] == 0xEE).all()
        got.append((out[o:o + n].tobytes(), bool(fl & 1), bool(fl & 2)))
    return got


def compare(lib, bodies, ref, labels=None):
    want = [R.outcome(b, ref) for b in bodies]
    got = host_rule(lib, bodies, ref, [len(w[0]) for w in want])
    for i, (body, g, w) in enumerate(zip(bodies, got, want)):
        assert g == w, (labels[i] if labels else i, g[0].hex(), w[0].hex())
        if w[1]:
            R.check_inverse(g[0], ref)
        else:
            assert g[0] == body
    return want


def test_the_ten_cases_by_hand(host):
    for ref, cigar, read, md, nm in LITERAL:
        body = M.make_record(cigar, ref if read is None else read, tags=b"XAi\x01\x02\x03\x04")
        new, done, had = R.outcome(body, [ref])
        assert done and not had and R.nm_md(new) == (nm, md), (ref, cigar, read, R.nm_md(new))
        assert new == body + b"NMC" + bytes([nm]) + b"MDZ" + md.encode() + b"\0"
        assert host_rule(host, [body], [ref], [len(new)]) == [(new, True, False)], (ref, cigar, read)
        R.check_inverse(new, [ref])
        # ... and at the end of a longer sequence, behind another one
        shifted = M.make_record(cigar, ref if read is None else read, tid=1, pos=3, flag=0x10, tags=b"NMC\x63MDZ99\0")
        new = R.calmd(shifted, ["GATTACA", "TTT" + ref])
        assert R.nm_md(new) == (nm, md) and len(new) == len(shifted) - 10 + 8 + len(md)
        assert host_rule(host, [shifted], ["GATTACA", "TTT" + ref], [len(new)]) == [(new, True, True)]


def test_crafted_records(host):
    labels, bodies, done = zip(*crafted())
    want = compare(host, list(bodies), genome(), labels)
    for label, body, d, w in zip(labels, bodies, done, want):
        assert w[1] == d, label
        assert label.startswith("skip:") != d or label == "cap passed", label
    by = dict(zip(labels, want))
    src = dict(zip(labels, bodies))
    # a few of the restatement's answers by hand, so that the yardstick is not only compared with itself
    xa, xb, xz = b"XAi\x01\x02\x03\x04", b"XBBs\x03\x00\x00\x00\x01\x00\x02\x00\x03\x00", b"XZZhello\0"
    tail = b"NMC\x00MDZ8\0"
    at = R.fields(src["tags first"])["tags_at"]
    assert by["tags first"][0][at:] == xa + xz + tail and by["tags in the middle"][0][at:] == xa + xz + xb + tail
    assert by["tags last"][0][at:] == xa + xz + tail and by["tags twice"][0][at:] == xa + xz + xb + xa + tail
    assert by["NM three times running"][0][at:] == xa + tail and by["other types"][0][at:] == xa + tail
    assert by["behind a B array"][0][at:] == xb + tail and by["no tags at all"][0][at:] == tail
    assert len(by["an old MD longer than the new one"][0]) < len(src["an old MD longer than the new one"])
    assert len(by["no tags at all"][0]) > len(src["no tags at all"])
    assert [R.nm_md(by["NM %d" % n][0]) for n in (255, 256, 65535, 65536)] == [(255, "2"), (256, "2"), (65535, "2"), (65536, "2")]
    assert [by["NM %d" % n][0][-9 - k:-5] for n, k in ((255, 0), (256, 1), (65535, 1), (65536, 3))] == [
        b"NMC\xff", b"NMS\x00\x01", b"NMS\xff\xff", b"NMI\x00\x00\x01\x00"]
    assert len(R.nm_md(by["cap met"][0])[1]) == 68 and R.nm_md(by["cap met"][0])[0] == 63
    assert R.nm_md(by["every base a mismatch"][0])[1].count("0") == 8 and R.nm_md(by["every base a mismatch"][0])[0] == 7
    assert R.nm_md(by["no base in the reference"][0]) == (3, "2N0N0N1") and R.nm_md(by["N above no base"][0]) == (4, "0T0N0N0N0")
    assert R.nm_md(by["IUPAC and = in the read"][0])[0] == 2
    assert R.nm_md(by["a run of ten and of a hundred"][0])[1].split(genome()[0][160])[0] == "10"
    assert "100" in R.nm_md(by["a run of ten and of a hundred"][0])[1]
    # had NM or MD: where the tags can be walked
    assert by["skip: CIGAR too short"][2] and by["skip: pos -1"][2] and by["skip: CG of type B"][2] and by["cap passed"][2]
    assert not by["skip: an unknown type"][2] and not by["skip: a string without its NUL"][2] and not by["skip: cut in the header"][2]


def test_the_records_of_mask_ends(host):
    """The crafted records of tests/test_mask_ends.py: every oddity of SEQ, CIGAR and place, NM and MD in front."""
    labels, bodies = zip(*mask_crafted())
    want = compare(host, list(bodies), genome(), labels)
    assert 40 < sum(w[1] for w in want) < len(want) - 20


def test_random_pool(host):
    bodies = pool()
    want = compare(host, bodies, genome())
    done = [w for w in want if w[1]]
    assert len(done) > 2500 and len(want) - len(done) > 100
    mds = [R.nm_md(w[0])[1] for w in done]
    assert sum("^" in m for m in mds) > 300 and sum("N" in m for m in mds) > 10 and sum(m.isdigit() for m in mds) > 100
    assert sum(len(w[0]) < len(b) for w, b in zip(want, bodies)) == 0 and sum(len(w[0]) > len(b) for w, b in zip(want, bodies)) > 2500
    # after the mask: every base of the windows N
    masked = [M.apply(b, 3, 2, M.ALL)[0] for b in bodies[:600]]
    want = compare(host, masked, genome())
    assert sum(R.nm_md(w[0])[0] >= 3 for w in want if w[1]) > 300


def test_growth_is_bounded(host):
    """No record grows by more than 7 + 3 + 2 * l_seq + 64 + 1 bytes, the figure of the bound call; the cap's record comes
    within the NM field's spare bytes of it."""
    assert host.kept_md_growth_host(0) == 75 and host.kept_md_growth_host(100) == 275
    most = -1 << 30
    for body in all_records():
        f = R.fields(body)
        new = R.calmd(body, genome())
        if new != body:
            assert len(new) - len(body) <= 75 + 2 * f["l_seq"]
            assert 2 * f["l_seq"] <= 4 * len(body) // 3
            most = max(most, len(new) - len(body) - 2 * f["l_seq"])
    assert most <= 75


def test_under_the_sanitizers(tmp_path):
    """The crafted records and a part of the pool through a program of its own built with -fsanitize=address,undefined:
    every record in a heap block of exactly its bytes, its new form in one of exactly the expected bytes."""
    exe = tmp_path / "calmd_walk"
    subprocess.check_call(["c++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "calmd_walk_main.cpp"), "-o", str(exe)])
    bases, contig_off = device_reference(genome())
    bodies = [c[1] for c in crafted()] + [c[1] for c in mask_crafted()] + pool()[:600]
    with open(tmp_path / "cases.bin", "wb") as out:
        out.write(struct.pack("<i", len(contig_off) - 1) + contig_off.tobytes() + bases.tobytes())
        for body in bodies:
            new, done, had = R.outcome(body, genome())
            out.write(struct.pack("<IIBBH", len(body), len(new), done, had, 0) + body + new)
    done = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, timeout=300)
    assert done.returncode == 0, done.stdout.decode()[-2000:] + done.stderr.decode()[-4000:]
    assert done.stdout.decode().splitlines()[-1] == "%d cases recomputed, 0 wrong" % len(bodies) and not done.stderr


# ---------------------------------------------------------------------- the command line
def test_options(tmp_path):
    out = tmp_path / "kept.bam"
    assert parse(tmp_path, "--write-kept", out, "--calmd").calmd is True
    assert parse(tmp_path, "--write-kept", out).calmd is False and parse(tmp_path).calmd is False


@pytest.mark.parametrize("extra", [
    ["--by-pmd-score", "--write-groups", "1", "--tag-group", "XG", "--tag-pmd-score", "DS", "--write-index", "--mask-ends", "2,1",
     "--mask-what", "mismatches"],
    ["--by-reference", "--min-mapq", "25", "--exclude-flags", "0x400", "-n", "0.5", "--downsample-seed", "7", "--mask-ends", "3"],
    ["-Q", "20", "--regions", "panel.bed", "--only-regions", "--chunk-mb", "64"],
    ["--by-reference", "--tag-group", "Nm"],
])
def test_allowed_combinations(tmp_path, extra):
    assert parse(tmp_path, "--write-kept", tmp_path / "kept.bam", "--calmd", *extra).calmd


def test_argument_errors(tmp_path, capsys):
    out = tmp_path / "kept.bam"
    assert "--calmd needs --write-kept" in error_of(tmp_path, capsys, "--calmd")
    assert "--tag-group NM with --calmd" in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "--by-reference", "--tag-group", "NM")
    assert "--tag-group MD with --calmd" in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "--by-reference", "--tag-group", "MD")
    for name in ("NM", "MD"):
        assert "--tag-pmd-score %s with --calmd" % name in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "--by-pmd-score",
                                                                   "--tag-pmd-score", name)
    # the restrictions of --write-kept stand as they are
    assert "--write-kept is written by the device decode path: not with --host-decode" in error_of(
        tmp_path, capsys, "--write-kept", out, "--calmd", "--host-decode")
    assert "--write-kept cannot be combined with --gpus 2" in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "--gpus", "2")
    assert "--write-kept cannot be combined with -n 1000" in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "-n", "1000")
    assert "--write-kept belongs to the tabulation pass" in error_of(tmp_path, capsys, "--write-kept", out, "--calmd", "--rescale-only")
