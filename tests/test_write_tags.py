"""--tag-group / --tag-pmd-score without a GPU: the rule of mapdamage_amd/csrc/mdx_kept_tags.h compiled for the host — the
score tag's bits against numpy's conversion, the tagged size against its restatement, the walk over a record's tags against
a strict parser of the test's own —, the same walk in a program of its own under the sanitizers, and the command line's options
and their argument errors."""

import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_gpu_write_kept import POOL, encode
from tests.test_write_kept import FLAG_FILTER_BITS, GROUP_KINDS, error_of, expected, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
TAG_BYTES = (0, 5, 7, 12)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("tags") / "write_tags_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "write_tags_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.tag_name_host.restype = lib.tag_none_host.restype = ctypes.c_uint32
    lib.tag_name_host.argtypes = [ctypes.c_char, ctypes.c_char]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------- the score tag's bits
def tag_bits(host, S):
    S = np.ascontiguousarray(S, np.int64)
    out = np.zeros(S.shape[0], np.uint32)
    host.pmd_tag_bits_host(ctypes.c_int64(S.shape[0]), ptr(S), ptr(out))
    return out


def numpy_bits(S):
    return (np.asarray(S, np.int64).astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)


def test_score_bits(host):
    one = 1 << 24
    values = [0, 1, -1]
    for v in (one + 1, one + 3, (1 << 25) + 1, (1 << 25) + 2, (1 << 25) + 6):        # ties to even, both directions
        values += [v, -v]
    for k in range(1, 201):                                                       # around 5.74 k: a long read's score
        centre = round(5.74 * one * k)
        values += [sign * (centre + d) for d in (-2, -1, 0, 1, 2) for sign in (1, -1)]
    for sign in (1, -1):
        values += [sign * (1 << 40) + (1 << 15) + d for d in (-1, 1)]
        values += [sign * ((1 << 40) + (1 << 16) + d) for d in (-1, 0, 1)]           # (half a unit in the last place up there)
    values += np.random.default_rng(24).integers(-(1 << 40) + 1, 1 << 40, 5000).tolist()
    values += np.random.default_rng(25).integers(-(1 << 27), 1 << 27, 2000).tolist()
    got, want = tag_bits(host, values), numpy_bits(values)
    np.testing.assert_array_equal(got, want)
    # what the numbers say: 0 is +0.0, the ties went to the even neighbour, the scaling lost nothing
    assert got[0] == 0 and got[1] == np.float32(2.0 ** -24).view(np.uint32)
    as_float = got.view(np.float32).astype(np.float64)
    assert as_float[3] == 1.0 and as_float[5] == 1.0 + 4 / one and as_float[4] == -1.0
    nearest = np.asarray(values, np.int64).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(as_float * one, nearest)
    assert np.abs(nearest - np.asarray(values, np.float64)).max() <= 2.0 ** 16


# ---------------------------------------------------------------------- the tagged size
def tagged_rule(host, flag, block_size, key, n_groups, selected, tag_bytes):
    flag = np.ascontiguousarray(flag, np.uint16)
    block_size = np.ascontiguousarray(block_size, np.uint32)
    key = np.ascontiguousarray(key, np.uint16)
    selected = None if selected is None else np.ascontiguousarray(selected, np.uint8)
    out = np.zeros(flag.shape[0], np.uint32)
    host.kept_tagged_bytes_host(ctypes.c_int64(flag.shape[0]), ptr(flag), ptr(key), ctypes.c_uint32(n_groups), ptr(selected),
                                ptr(block_size), ctypes.c_uint32(tag_bytes), ptr(out))
    return out


def tagged_expected(flag, block_size, key, n_groups, selected, tag_bytes):
    """The untagged rule (tests/test_write_kept.py), then: with tags no record without a key, and tag_bytes more."""
    base = expected(flag, block_size, key, n_groups, selected).astype(np.int64)
    if tag_bytes:
        base = np.where((base > 0) & (np.asarray(key, np.int64) != 0xFFFF), base + tag_bytes, 0)
    return base.astype(np.uint32)


@pytest.mark.parametrize("tag_bytes", TAG_BYTES)
def test_size_rule_flag_bits(host, tag_bytes):
    flags = [0] + [1 << b for b in range(16)] + [0x200 | 0x1, 0x200 | 0x10 | 0x40, 0x200 | 0xC000, 0x1 | 0x2 | 0x10 | 0x40 | 0x80,
                                                 0xC000, 0xF04, 0xFFFF]
    bs = np.full(len(flags), 100, np.uint32)
    key = np.arange(len(flags)) % 3
    got = tagged_rule(host, flags, bs, key, 3, None, tag_bytes)
    np.testing.assert_array_equal(got, tagged_expected(flags, bs, key, 3, None, tag_bytes))
    assert [int(g) for f, g in zip(flags, got) if not f & 0xF04] == [104 + tag_bytes] * sum(1 for f in flags if not f & 0xF04)
    assert not any(g for f, g in zip(flags, got) if f & 0xF04)
    bs = np.array([33, 32, 37, 65535, 65536, 2**31 - 20], np.uint32)
    np.testing.assert_array_equal(tagged_rule(host, np.zeros(6, np.uint16), bs, np.zeros(6), 1, None, tag_bytes), bs.astype(np.int64) + 4 + tag_bytes)


@pytest.mark.parametrize("tag_bytes", TAG_BYTES)
@pytest.mark.parametrize("n_groups", [1, 2, 3, 65535])
def test_size_rule_groups(host, n_groups, tag_bytes):
    rng = np.random.default_rng(n_groups)
    n_lib = max(1, min(4, 65535 // n_groups))
    key = (rng.integers(0, n_lib, 4000) * n_groups + rng.integers(0, n_groups, 4000)).astype(np.uint16)
    key[::17] = 0xFFFF
    flag = np.where(rng.random(4000) < 0.3, rng.choice(FLAG_FILTER_BITS, 4000), 0).astype(np.uint16) | 0x10
    bs = rng.integers(33, 500, 4000).astype(np.uint32)
    for selected in (None, np.ones(n_groups, np.uint8), np.zeros(n_groups, np.uint8), (np.arange(n_groups) % 2 == 0).astype(np.uint8),
                     (np.arange(n_groups) == n_groups - 1).astype(np.uint8)):
        got = tagged_rule(host, flag, bs, key, n_groups, selected, tag_bytes)
        np.testing.assert_array_equal(got, tagged_expected(flag, bs, key, n_groups, selected, tag_bytes))
        # a record without a key: never with a selection, never with a tag; written as it is where neither is asked for
        assert got[::17].any() == (selected is None and tag_bytes == 0)
        written = got > 0
        np.testing.assert_array_equal(got[written], bs[written].astype(np.int64) + 4 + tag_bytes)
    assert tagged_rule(host, flag, bs, key, n_groups, None, tag_bytes).any()


# ---------------------------------------------------------------------- the walk over a record's tags
SCALARS = {"A": b"x", "c": b"\xfe", "C": b"\xfe", "s": b"\x01\x80", "S": b"\x01\x80", "i": b"\x01\x02\x03\x84", "I": b"\x01\x02\x03\x84",
           "f": struct.pack("<f", -1.5)}
WIDTH = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
MALFORMED = " (malformed)"
SOUGHT = {"XG": b"XGS\x03\x00", "DS": b"DSf" + struct.pack("<f", 2.5)}


def tag(name, ty, payload):
    return name.encode() + ty.encode() + payload


def b_array(name, sub, count, fill=None):
    payload = POOL[1000:1000 + WIDTH[sub] * count] if fill is None else fill
    assert len(payload) == WIDTH[sub] * count
    return tag(name, "B", sub.encode() + struct.pack("<I", count) + payload)


def strict_names(region):
    """The names of a well-formed tag region, by a parser of the test's own: every tag complete, nothing left over."""
    names, at = [], 0
    while at < len(region):
        assert at + 3 <= len(region)
        names.append(region[at:at + 2].decode())
        ty = chr(region[at + 2])
        at += 3
        if ty in "ZH":
            at = region.index(b"\0", at) + 1
        elif ty == "B":
            sub, count = chr(region[at]), struct.unpack_from("<I", region, at + 1)[0]
            at += 5 + WIDTH[sub] * count
        else:
            at += len(SCALARS[ty])
    assert at == len(region)
    return names


def well_formed_regions():
    """(what, region) of well-formed tag regions that hold neither XG nor DS."""
    out = [("no tags", b""), ("RG:Z", b"RGZrgA\0"), ("an empty Z", b"XZZ\0"), ("an H", b"XHH1AE301\0"),
           ("a long XA:Z", tag("XA", "Z", bytes(33 + b % 90 for b in POOL[300:700]) + b"\0"))]
    out += [("B:i of %d" % k, b_array("ZB", "i", k)) for k in range(9)]
    out += [("B:%s" % sub, b_array("ZB", sub, 5)) for sub in WIDTH]
    out += [("scalar %s" % ty, tag("Y" + ty.upper(), ty, payload)) for ty, payload in SCALARS.items()]
    # the sought names where they are no names: in a string's payload, in an array's payload, split over two tags
    out.append(("XG in a Z payload", tag("XA", "Z", b"chr1,XGS,DSf,+100\0")))
    out.append(("DS in an H payload", tag("XH", "H", b"DSf0XGS0\0")))
    out.append(("XG in a B:C payload", b_array("ZB", "C", 8, b"XGS\x01\x00DSf")))
    out.append(("DS in a B:s payload", b_array("ZB", "s", 4, b"DSfXGSxx")))
    out.append(("XG in a B:i payload", b_array("ZB", "i", 2, b"XGSxDSfx")))
    out.append(("X then G", tag("AX", "C", b"G") + tag("SX", "A", b"D") + tag("SD", "c", b"S")))
    out.append(("the type byte", tag("AB", "A", b"X") + tag("GX", "C", b"\0")))
    everything = b"".join(region for _, region in out)
    out.append(("all of them", everything))
    return out


def malformed_regions():
    """(what, region): the walk cannot follow these to their end — it stops, whatever lies behind, and reports no clash."""
    xg = SOUGHT["XG"]
    return [("an unknown type", tag("QQ", "q", b"\1\2\3\4") + xg),
            ("an unknown type behind a tag", b"RGZrgA\0" + tag("QQ", "?", b"") + xg),
            ("a lower-case z", tag("QQ", "z", b"abc\0") + xg),
            ("a name cut", b"RGZrgA\0X"), ("a type cut", b"RGZrgA\0XG"), ("two bytes", b"XG"), ("one byte", b"D"),
            ("a scalar cut", tag("YI", "I", b"\1\2")), ("a scalar cut by a byte", tag("YF", "f", b"\1\2\3")),
            ("a short cut", b"RGZrgA\0" + tag("YS", "s", b"\1")), ("an A without its byte", tag("YA", "A", b"")),
            ("a Z without its end", tag("XA", "Z", b"chr1,XGS,DSf")), ("a Z without a payload", tag("XA", "Z", b"")),
            ("a B header cut", tag("ZB", "B", b"i\x02\0\0")), ("a B without a header", tag("ZB", "B", b"")),
            ("a B past the end", tag("ZB", "B", b"i" + struct.pack("<I", 3) + b"\0" * 11)),
            ("a B past the end by far", tag("ZB", "B", b"i" + struct.pack("<I", 0xFFFFFFFF) + xg)),
            ("a B of 2^30 words", tag("ZB", "B", b"I" + struct.pack("<I", 1 << 30) + xg + xg)),
            ("a B of an unknown subtype past the end", tag("ZB", "B", b"q" + struct.pack("<I", 2) + b"\0" * 7))]


def all_regions():
    """(what, region, is a clash) for the walk, well-formed and not."""
    cases = [(what, region, False) for what, region in well_formed_regions()]
    plain = [region for _, region in well_formed_regions()[:-1]]
    for name, sought in SOUGHT.items():
        cases.append((name + " alone", sought, True))
        for k, region in enumerate(plain):
            if not region:
                continue
            other = plain[(k + 7) % len(plain)]
            cases += [("%s first, case %d" % (name, k), sought + region, True), ("%s last, case %d" % (name, k), region + sought, True),
                      ("%s in the middle, case %d" % (name, k), region + sought + other, True)]
        # (the name decides, whatever its type)
        cases += [(name + " as a Z", b"RGZrgA\0" + tag(name, "Z", b"x\0"), True), (name + " as a B", b_array(name, "c", 3) + b"RGZrgA\0", True)]
    cases.append(("both", b"RGZrgA\0" + SOUGHT["DS"] + SOUGHT["XG"], True))
    cases += [(what + MALFORMED, region, False) for what, region in malformed_regions()]
    # ... but a clash in front of the place where the walk loses its way is one
    cases += [("XG in front of: " + what + MALFORMED, SOUGHT["XG"] + region, True) for what, region in malformed_regions()]
    return cases


def record_has(host, body, names):
    buf = np.frombuffer(body, np.uint8).copy()
    ids = [host.tag_name_host(n[0].encode(), n[1].encode()) if n else host.tag_none_host() for n in names]
    return bool(host.record_has_tag_host(ptr(buf), ctypes.c_uint32(len(body)), ctypes.c_uint32(ids[0]), ctypes.c_uint32(ids[1])))


def test_walk(host):
    assert host.tag_name_host(b"X", b"G") == ord("X") | ord("G") << 8 and host.tag_none_host() > 0xFFFF
    for what, region in well_formed_regions():
        assert not {"XG", "DS"} & set(strict_names(region)), what
    n_clash = 0
    for k, (what, region, clash) in enumerate(all_regions()):
        # the record around the region: the encoder's, names and sequences of every length, no tags of its own
        body = encode(k, tag=0) + region
        if not what.endswith(MALFORMED):
            assert bool({"XG", "DS"} & set(strict_names(region))) == clash, what
        assert record_has(host, body, ("XG", "DS")) == clash, what
        assert record_has(host, body, ("DS", "XG")) == clash, what
        # one name asked for: the other one is a tag like any other
        has = {name: clash and (what.startswith(name) or what == "both") for name in SOUGHT}
        for name in SOUGHT:
            assert record_has(host, body, (name, None)) == has[name], (what, name)
            assert record_has(host, body, (None, name)) == has[name], (what, name)
        assert not record_has(host, body, (None, None)), what
        assert not record_has(host, body, ("MR", "xg")), what
        n_clash += clash
    assert n_clash > 150
    # the encoder's own tags (RG:Z, a B:i array of 0 to 8 entries, a long XA:Z) in front of the sought one, and without it
    for i in range(72):
        body = encode(i)
        assert not record_has(host, body, ("XG", "DS")), i
        assert record_has(host, body, ("XA", None)) == (i % 4 == 3) and record_has(host, body, (None, "ZB")) == (i % 4 == 2), i
        assert record_has(host, body + SOUGHT["DS"], ("XG", "DS")) and not record_has(host, body + SOUGHT["DS"], ("XG", None)), i
    # a record whose fields point behind its end (l_seq): no tag region, no read, no clash
    body = bytearray(encode(3, tag=0) + SOUGHT["XG"])
    assert record_has(host, bytes(body), ("XG", None))
    body[16:20] = struct.pack("<I", 0xFFFFFFF0)
    assert not record_has(host, bytes(body), ("XG", None))


def test_walk_under_the_sanitizers(tmp_path):
    """The same regions through a program of its own built with -fsanitize=address,undefined: every region in a heap block of
    exactly its size."""
    exe = tmp_path / "walk"
    subprocess.check_call(["c++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "write_tags_walk_main.cpp"), "-o", str(exe)])
    cases = all_regions()
    with open(tmp_path / "regions.bin", "wb") as out:
        for _, region, clash in cases:
            out.write(struct.pack("<BI", int(clash), len(region)) + region)
    done = subprocess.run([str(exe), str(tmp_path / "regions.bin")], capture_output=True, timeout=120)
    assert done.returncode == 0, done.stdout.decode()[-2000:] + done.stderr.decode()[-4000:]
    assert done.stdout.decode().splitlines()[-1] == "%d regions walked, 0 wrong" % len(cases) and not done.stderr


# ---------------------------------------------------------------------- the command line
@pytest.mark.parametrize("kind", sorted(GROUP_KINDS))
def test_group_tag_with_every_kind_of_groups(tmp_path, kind):
    out = tmp_path / "kept.bam"
    o = parse(tmp_path, "--write-kept", out, "--tag-group", "XG", *GROUP_KINDS[kind])
    assert o.tag_group == "XG" and o.tag_pmd_score is None and o.write_groups is None
    o = parse(tmp_path, "--write-kept", out, "--tag-group", "g0", "--write-groups", "1,0", *GROUP_KINDS[kind])
    assert o.tag_group == "g0" and o.write_groups == (0, 1)


def test_score_tag_options(tmp_path):
    out = tmp_path / "kept.bam"
    o = parse(tmp_path, "--write-kept", out, "--by-pmd-score", "--tag-pmd-score", "DS")
    assert o.tag_pmd_score == "DS" and o.tag_group is None
    o = parse(tmp_path, "--write-kept", out, "--by-pmd-score", "--pmd-thresholds", "0,3", "--tag-pmd-score", "DS", "--tag-group", "XG")
    assert (o.tag_group, o.tag_pmd_score) == ("XG", "DS")
    o = parse(tmp_path, "--write-kept", out, "--by-pmd-score", "--tag-pmd-score", "d9", "--tag-group", "D9", "--write-groups", "1")
    assert (o.tag_group, o.tag_pmd_score, o.write_groups) == ("D9", "d9", (1,))


@pytest.mark.parametrize("extra", [
    ["-Q", "20", "--by-reference"], ["--regions", "panel.bed", "--only-regions"], ["--regions", "panel.bed", "--write-groups", "0"],
    ["--by-terminal-damage", "--min-mapq", "25", "--exclude-flags", "0x400", "-n", "0.5", "--downsample-seed", "7"],
    ["--by-reference", "--merge-libraries", "--chunk-mb", "64"],
])
def test_allowed_combinations(tmp_path, extra):
    o = parse(tmp_path, "--write-kept", tmp_path / "kept.bam", "--tag-group", "XG", *extra)
    assert o.tag_group == "XG"


def test_allowed_with_the_estimate(tmp_path):
    from mapdamage_amd.main import parse_args
    o = parse_args(["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out"), "--write-kept", str(tmp_path / "kept.bam"), "--stats",
                    "--fix-nicks", "--by-pmd-score", "--tag-group", "XG", "--tag-pmd-score", "DS"])
    assert o.want_stats and (o.tag_group, o.tag_pmd_score) == ("XG", "DS")


def test_defaults(tmp_path):
    for args in ([], ["--write-kept", tmp_path / "kept.bam"], ["--write-kept", tmp_path / "kept.bam", "--by-pmd-score", "--write-groups", "1"]):
        o = parse(tmp_path, *args)
        assert o.tag_group is None and o.tag_pmd_score is None
    plain, tagged = parse(tmp_path, "--write-kept", tmp_path / "k.bam", "--by-pmd-score"), parse(
        tmp_path, "--write-kept", tmp_path / "k.bam", "--by-pmd-score", "--tag-group", "XG", "--tag-pmd-score", "DS")
    differ = {k for k in vars(tagged) if k not in ("record_filter",) and vars(plain).get(k) != vars(tagged)[k]}
    assert differ == {"tag_group", "tag_pmd_score"}


def test_argument_errors(tmp_path, capsys):
    out = tmp_path / "kept.bam"
    assert "--tag-group needs --write-kept" in error_of(tmp_path, capsys, "--by-reference", "--tag-group", "XG")
    assert "--tag-pmd-score needs --write-kept" in error_of(tmp_path, capsys, "--by-pmd-score", "--tag-pmd-score", "DS")
    assert "--tag-group needs a run with groups" in error_of(tmp_path, capsys, "--write-kept", out, "--tag-group", "XG")
    message = error_of(tmp_path, capsys, "--write-kept", out, "--by-reference", "--tag-pmd-score", "DS")
    assert "--tag-pmd-score needs --by-pmd-score" in message
    for bad in ("X", "XGG", "1G", "X_", "X:", "XG:S", "", "éa"):
        assert "--tag-group %s: a tag is two characters, [A-Za-z][A-Za-z0-9]" % bad in error_of(
            tmp_path, capsys, "--write-kept", out, "--by-reference", "--tag-group=" + bad)
        assert "--tag-pmd-score %s: a tag is two characters" % bad in error_of(
            tmp_path, capsys, "--write-kept", out, "--by-pmd-score", "--tag-pmd-score=" + bad)
    message = error_of(tmp_path, capsys, "--write-kept", out, "--by-pmd-score", "--tag-group", "XG", "--tag-pmd-score", "XG")
    assert "--tag-group and --tag-pmd-score name the same tag, XG" in message
    # the restrictions of --write-kept stand as they are
    assert "--write-kept is written by the device decode path: not with --host-decode" in error_of(
        tmp_path, capsys, "--write-kept", out, "--by-reference", "--tag-group", "XG", "--host-decode")
    assert "--write-kept cannot be combined with --gpus 2" in error_of(tmp_path, capsys, "--write-kept", out, "--by-reference", "--tag-group", "XG",
                                                                     "--gpus", "2")
    assert "--write-kept cannot be combined with -n 1000" in error_of(tmp_path, capsys, "--write-kept", out, "--by-reference", "--tag-group", "XG",
                                                                    "-n", "1000")
    assert "cannot be combined with -Q" in error_of(tmp_path, capsys, "--write-kept", out, "--by-pmd-score", "--tag-pmd-score", "DS", "-Q", "20")
