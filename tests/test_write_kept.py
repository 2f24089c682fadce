"""--write-kept without a GPU: the selection rule of mapdamage_amd/csrc/mdx_kept.h compiled for the host against its
restatement in numpy, and the command line's options, their list parser and their argument errors."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_FILTER_BITS = (0x4, 0x100, 0x200, 0x400, 0x800)


@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("kept") / "kept_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mapdamage_amd", "csrc"),
                           os.path.join(ROOT, "tests", "kept_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))

    def rule(flag, block_size, key=None, n_groups=0, selected=None):
        flag = np.ascontiguousarray(flag, np.uint16)
        block_size = np.ascontiguousarray(block_size, np.uint32)
        key = None if key is None else np.ascontiguousarray(key, np.uint16)
        selected = None if selected is None else np.ascontiguousarray(selected, np.uint8)
        out = np.zeros(flag.shape[0], np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)       # noqa: E731
        lib.kept_bytes_host(ctypes.c_int64(flag.shape[0]), ptr(flag), ptr(key), ctypes.c_uint32(n_groups), ptr(selected),
                            ptr(block_size), ptr(out))
        return out
    return rule


def expected(flag, block_size, key=None, n_groups=0, selected=None):
    """The rule once more: counted, in a listed group if there is a list, then block_size + 4."""
    flag = np.asarray(flag, np.int64)
    keep = (flag & 0xF04) == 0
    if selected is not None:
        key = np.asarray(key, np.int64)
        sel = np.asarray(selected, bool)
        keep &= key != 0xFFFF
        keep &= sel[np.where(key == 0xFFFF, 0, key) % n_groups]
    return np.where(keep, np.asarray(block_size, np.int64) + 4, 0).astype(np.uint32)


def test_rule_flag_bits(host_rule):
    # every bit of the sixteen alone, the five of 0xF04 among them; 0x200 beside bits that drop nothing; the hint bits
    flags = [0] + [1 << b for b in range(16)] + [0x200 | 0x1, 0x200 | 0x10 | 0x40, 0x200 | 0xC000, 0x1 | 0x2 | 0x10 | 0x40 | 0x80,
                                                 0xC000, 0xF04, 0xFFFF]
    bs = np.full(len(flags), 100, np.uint32)
    got = host_rule(flags, bs)
    np.testing.assert_array_equal(got, expected(flags, bs))
    for bit in FLAG_FILTER_BITS:
        assert got[1 + bit.bit_length() - 1] == 0, hex(bit)
    kept = [f for f, g in zip(flags, got) if g]
    assert kept == [f for f in flags if not f & 0xF04] and 0xC000 in kept and 0x1 in kept


def test_rule_block_sizes(host_rule):
    bs = np.array([33, 32, 37, 65535, 65536, 2**31 - 5], np.uint32)
    got = host_rule(np.zeros(len(bs), np.uint16), bs)
    np.testing.assert_array_equal(got, bs.astype(np.int64) + 4)
    assert got[0] == 37 and int(got[-1]) == 2**31 - 1
    np.testing.assert_array_equal(host_rule(np.full(len(bs), 0x400, np.uint16), bs), 0)


@pytest.mark.parametrize("n_groups", [1, 2, 3, 65535])
def test_rule_groups(host_rule, n_groups):
    rng = np.random.default_rng(n_groups)
    n_lib = max(1, min(4, 65535 // n_groups))
    lib = rng.integers(0, n_lib, 4000)
    group = rng.integers(0, n_groups, 4000)
    key = (lib * n_groups + group).astype(np.uint16)
    key[::17] = 0xFFFF
    flag = np.where(rng.random(4000) < 0.3, rng.choice(FLAG_FILTER_BITS, 4000), 0).astype(np.uint16) | 0x10
    bs = rng.integers(33, 500, 4000).astype(np.uint32)
    for selected in (np.ones(n_groups, np.uint8), np.zeros(n_groups, np.uint8), (np.arange(n_groups) % 2 == 0).astype(np.uint8),
                     (np.arange(n_groups) == n_groups - 1).astype(np.uint8)):
        got = host_rule(flag, bs, key, n_groups, selected)
        np.testing.assert_array_equal(got, expected(flag, bs, key, n_groups, selected))
        # the one case the header specifies for that key: never written with a selection
        assert not got[::17].any()
        assert not got[~selected.astype(bool)[np.where(key == 0xFFFF, 0, key.astype(np.int64)) % n_groups]].any()
    # without a selection the key says nothing, 0xFFFF included
    np.testing.assert_array_equal(host_rule(flag, bs, key, n_groups, None), expected(flag, bs))
    assert host_rule(flag, bs, key, n_groups, None)[::17].any()


def test_rule_selected_and_not(host_rule):
    # two libraries x three groups, group 1 listed: keys 1 and 4 stay
    key = np.arange(6, dtype=np.uint16)
    got = host_rule(np.zeros(6, np.uint16), np.full(6, 40, np.uint32), key, 3, np.array([0, 1, 0], np.uint8))
    np.testing.assert_array_equal(got, [0, 44, 0, 0, 44, 0])


# ---- the command line


def parse(tmp_path, *args, inp="x.bam"):
    from mapdamage_amd.main import parse_args
    return parse_args(["-i", str(inp), "-r", "ref.fa", "-d", str(tmp_path / "out"), "--no-stats"] + [str(a) for a in args])


GROUP_KINDS = {
    "by-reference": ["--by-reference"],
    "reference-groups": ["--reference-groups", "groups.tsv"],
    "regions": ["--regions", "panel.bed"],
    "region-groups": ["--region-groups", "panels.bed"],
    "terminal-damage": ["--by-terminal-damage"],
    "pmd": ["--by-pmd-score", "--pmd-thresholds", "1,3"],
}


@pytest.mark.parametrize("kind", sorted(GROUP_KINDS))
def test_options_with_every_kind_of_groups(tmp_path, kind):
    out = tmp_path / "kept.bam"
    o = parse(tmp_path, "--write-kept", out, *GROUP_KINDS[kind])
    assert o.write_kept == out and o.write_groups is None
    o = parse(tmp_path, "--write-kept", out, "--write-groups", "2,0", *GROUP_KINDS[kind])
    assert o.write_groups == (0, 2)
    o = parse(tmp_path, "--write-kept", out, "--write-groups", " 1 ", *GROUP_KINDS[kind])
    assert o.write_groups == (1,)


def test_options_without_groups_and_absent(tmp_path):
    o = parse(tmp_path, "--write-kept", tmp_path / "kept.bam")
    assert o.write_kept == tmp_path / "kept.bam" and o.write_groups is None
    o = parse(tmp_path)
    assert o.write_kept is None and o.write_groups is None


@pytest.mark.parametrize("extra", [
    ["-Q", "20"], ["--merge-libraries"], ["-l", "50", "-m", "20"], ["-a", "5", "-b", "5"], ["--chunk-mb", "64"],
    ["--min-mapq", "25", "--exclude-flags", "0x400", "--require-flags", "1", "--min-read-length", "30", "--max-read-length", "200"],
    ["-n", "0.5", "--downsample-seed", "7"], ["--regions", "panel.bed", "--only-regions"],
    ["--regions", "panel.bed", "--only-regions", "--write-groups", "0"],
])
def test_allowed_combinations(tmp_path, extra):
    o = parse(tmp_path, "--write-kept", tmp_path / "kept.bam", *extra)
    assert o.write_kept is not None


@pytest.mark.parametrize("extra", [["--stats", "--fix-nicks"], ["--rescale", "--fix-nicks"]])
def test_allowed_with_the_estimate(tmp_path, extra):
    from mapdamage_amd.main import parse_args
    o = parse_args(["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out"), "--write-kept", str(tmp_path / "kept.bam")] + extra)
    assert o.write_kept is not None and o.want_stats


def test_list_parser():
    from mapdamage_amd.main import check_write_groups, parse_write_groups
    assert parse_write_groups("0") == (0,)
    assert parse_write_groups("3,1,2") == (1, 2, 3)
    assert parse_write_groups("10, 2") == (2, 10)
    for text, what in (("", "empty entry"), ("1,,2", "empty entry"), ("1,", "empty entry"), ("a", "not an integer"),
                       ("1,chr1", "not an integer"), ("1.5", "not an integer"), ("0x1", "not an integer"),
                       ("-1", "negative"), ("2,-3", "negative"), ("1,1", "listed twice"), ("2,0,2", "listed twice")):
        with pytest.raises(ValueError, match=what):
            parse_write_groups(text)
    check_write_groups((0, 3), 4)
    with pytest.raises(ValueError, match=r"group index 4 is outside 0\.\.3"):
        check_write_groups((0, 4), 4)


def error_of(tmp_path, capsys, *args, inp="x.bam", base=("--no-stats",)):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as err:
        parse_args(["-i", str(inp), "-r", "ref.fa", "-d", str(tmp_path / "out")] + list(base) + [str(a) for a in args])
    assert err.value.code == 2
    return capsys.readouterr().err


def test_argument_errors(tmp_path, capsys):
    out = tmp_path / "kept.bam"
    assert "--write-groups needs --write-kept" in error_of(tmp_path, capsys, "--by-reference", "--write-groups", "0")
    assert "--write-groups needs a run with groups" in error_of(tmp_path, capsys, "--write-kept", out, "--write-groups", "0")
    assert "--write-kept is written by the device decode path: not with --host-decode" in error_of(
        tmp_path, capsys, "--write-kept", out, "--host-decode")
    message = error_of(tmp_path, capsys, "--write-kept", out, "--gpus", "2")
    assert "--write-kept cannot be combined with --gpus 2" in message and "one file has one order" in message
    message = error_of(tmp_path, capsys, "--write-kept", out, "-n", "1000")
    assert "--write-kept cannot be combined with -n 1000" in message and "reservoir" in message
    assert "--write-kept cannot be combined with -n 1" in error_of(tmp_path, capsys, "--write-kept", out, "-n", "1")
    assert "--write-kept belongs to the tabulation pass" in error_of(tmp_path, capsys, "--write-kept", out, "--rescale-only", base=())
    assert "--write-kept belongs to the tabulation pass" in error_of(tmp_path, capsys, "--write-kept", out, "--stats-only",
                                                                    "--fix-nicks", base=())
    assert "its directory does not exist" in error_of(tmp_path, capsys, "--write-kept", tmp_path / "missing" / "kept.bam")
    for text, what in (("1,,2", "--write-groups: an empty entry"), ("x", "--write-groups: 'x' is not an integer"),
                       ("0,-2", "--write-groups: group index -2 is negative"), ("1,1", "--write-groups: group index 1 is listed twice")):
        assert what in error_of(tmp_path, capsys, "--write-kept", out, "--by-pmd-score", "--write-groups=" + text)


def test_output_must_not_be_the_input(tmp_path, capsys):
    inp = tmp_path / "in.bam"
    inp.write_bytes(b"")
    assert "is the input file" in error_of(tmp_path, capsys, "--write-kept", inp, inp=inp)
    link = tmp_path / "link.bam"
    link.symlink_to(inp)
    assert "is the input file" in error_of(tmp_path, capsys, "--write-kept", link, inp=inp)
    # another existing file, and a path that does not exist yet, are fine
    other = tmp_path / "other.bam"
    other.write_bytes(b"")
    assert parse(tmp_path, "--write-kept", other, inp=inp).write_kept == other
    assert parse(tmp_path, "--write-kept", tmp_path / "new.bam", inp=inp).write_kept == tmp_path / "new.bam"
