"""--depth, the parts that need no GPU: the rule (mapdamage_amd/csrc/mdx_depth_key.h compiled for the host as the stand-alone
program tests/depth_key_host.cpp, once more under AddressSanitizer and UBSan, against the brute force of tests/depth_rule.py),
the command line's argument errors and the emitters of mapdamage_amd/depth.py.  The device stage: tests/test_gpu_depth.py."""

import os
import subprocess

import numpy as np
import pytest

from tests import depth_rule as PR
from tests.dup_rule import columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8
UNKNOWN = 0xFFFF

# ---------------------------------------------------------------------- the hand-written records (the GPU test runs them too)
HAND_LENGTHS = [500, 300]
HAND_LIBRARIES = 3
HAND = [
    # (record, kind, intervals)
    ((0, 0, 0, 10, [(M, 30), (I, 2), (M, 30)]), PR.COUNTED, [(10, 70)]),
    ((0, 1, 0, 100, [(M, 20), (D, 5), (M, 20)]), PR.COUNTED, [(100, 120), (125, 145)]),
    ((0, 2, 0, 200, [(M, 10), (D, 3), (N, 4), (EQ, 10)]), PR.COUNTED, [(200, 210), (217, 227)]),
    ((0x10, 0, 0, 300, [(S, 5), (M, 50), (H, 5)]), PR.COUNTED, [(300, 350)]),
    ((0, 0, 0, 50, [(S, 5), (H, 5)]), PR.OUTSIDE, []),                            # clips only
    ((0, 0, 0, 50, []), PR.OUTSIDE, []),                                          # no CIGAR
    ((0, 0, 0, 50, [(I, 7)]), PR.OUTSIDE, []),                                    # nothing on the reference
    ((0, 0, 0, 400, [(D, 3), (M, 10)]), PR.COUNTED, [(403, 413)]),                # D first
    ((0, 0, 0, 420, [(M, 10), (N, 5)]), PR.COUNTED, [(420, 430)]),                # N last
    ((0, 0, 0, 440, [(M, 5), (EQ, 5), (X, 5)]), PR.COUNTED, [(440, 455)]),        # abutting M = X
    ((0, 0, 0, 456, [(M, 5), (P, 2), (I, 1), (S, 0), (M, 5)]), PR.COUNTED, [(456, 466)]),
    ((0, 0, 0, 480, [(M, 20)]), PR.COUNTED, [(480, 500)]),                        # ends exactly at the sequence's end
    ((0, 0, 0, 481, [(M, 20)]), PR.OUTSIDE, []),                                  # one base beyond
    ((0, 0, 0, 490, [(M, 10), (N, 1)]), PR.OUTSIDE, []),                          # ... by an N alone
    ((0, 0, 0, -1, [(M, 20)]), PR.OUTSIDE, []),
    ((0, 0, -1, 5, [(M, 20)]), PR.OUTSIDE, []),
    ((0, 0, 2, 5, [(M, 20)]), PR.OUTSIDE, []),                                    # tid = n_contig
    ((0, 0, 1, 5, [(N, 4)]), PR.COUNTED, []),                                     # a reference base, none covered
    ((0, 0, 1, 0, [(M, 300)]), PR.COUNTED, [(0, 300)]),                           # a whole sequence
    ((0, 0, 1, 299, [(M, 1)]), PR.COUNTED, [(299, 300)]),
    ((0, UNKNOWN, 0, 10, [(M, 20)]), PR.IGNORED, []),                             # a read group nobody knows
    ((0, 3, 0, 10, [(M, 20)]), PR.IGNORED, []),                                   # no library of the context's three
] + [((bit, 0, 0, 10, [(M, 20)]), PR.IGNORED, []) for bit in (0x4, 0x100, 0x200, 0x400, 0x800)] + [
    ((0x404, UNKNOWN, -1, -1, []), PR.IGNORED, []),                               # the filter comes first
    ((0x1 | 0x20 | 0x40, 0, 0, 10, [(M, 20)]), PR.COUNTED, [(10, 30)]),           # a paired record is a record
]


# ---------------------------------------------------------------------- the rule
@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def host_rule(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("depth_key") / "depth_key_host"
    subprocess.check_call(["g++", *request.param, "-I", CSRC, os.path.join(ROOT, "tests", "depth_key_host.cpp"), "-o", str(exe)])

    def rule(records, n_libraries, lengths, cigar_off=None, n_cigar=None):
        flag, lib, tid, pos, off, cigar = columns(records)
        off = off if cigar_off is None else np.asarray(cigar_off, np.uint32)
        text = ["%d %d %d %d %d" % (len(lengths), n_libraries, len(records), len(cigar), len(cigar) if n_cigar is None else n_cigar),
                " ".join(str(int(x)) for x in lengths)]
        text += ["%d %d %d %d" % row for row in zip(flag.tolist(), lib.tolist(), tid.tolist(), pos.tolist())]
        text += [" ".join(str(int(x)) for x in off), " ".join(str(int(x)) for x in cigar)]
        out = subprocess.run([str(exe)], input=("\n".join(text) + "\n").encode(), capture_output=True, timeout=120)
        assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
        assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
        lines = out.stdout.decode().split("\n")
        assert lines[-2] == "OK" and len(lines) == len(records) + 2
        rows = [[int(x) for x in line.split()] for line in lines[:len(records)]]
        return [r[0] for r in rows], [list(zip(r[1::2], r[2::2])) for r in rows]
    return rule


def test_hand_written_records(host_rule):
    records = [r for r, _, _ in HAND]
    kinds, ivs = host_rule(records, HAND_LIBRARIES, HAND_LENGTHS)
    assert kinds == [k for _, k, _ in HAND]
    assert ivs == [iv for _, _, iv in HAND]
    # ... and the restated rule says the same
    assert [PR.classify(*r, HAND_LIBRARIES, HAND_LENGTHS) for r in records] == kinds
    assert [PR.intervals(r[3], r[4]) if k == PR.COUNTED else [] for r, k in zip(records, kinds)] == ivs


def test_clamped_cigar_offsets(host_rule):
    """Offsets beyond the CIGAR column are clamped to it: the record has the operations that are there, or none."""
    two = [(0, 0, 0, 10, [(M, 5)]), (0, 0, 0, 10, [(M, 5), (D, 3), (M, 2)])]
    kinds, ivs = host_rule(two, 1, [100], cigar_off=[0, 1, 9], n_cigar=2)
    assert kinds == [PR.COUNTED, PR.COUNTED] and ivs == [[(10, 15)], [(10, 15)]]         # (M 5 alone: the D lies at the column's end)
    kinds, ivs = host_rule(two, 1, [100], cigar_off=[0, 1, 9], n_cigar=3)
    assert ivs == [[(10, 15)], [(10, 15)]]                                               # (M 5, D 3: one interval)
    kinds, ivs = host_rule(two, 1, [100], cigar_off=[5, 7, 9], n_cigar=4)
    assert kinds == [PR.OUTSIDE, PR.OUTSIDE] and ivs == [[], []]
    kinds, ivs = host_rule(two, 1, [100], cigar_off=[3, 1, 4])                            # (an offset behind its successor: none)
    assert kinds == [PR.OUTSIDE, PR.COUNTED] and ivs == [[], [(10, 15), (18, 20)]]


def random_cigar(rng):
    shape = rng.integers(0, 10)
    clip = lambda: [[], [(S, int(rng.integers(1, 9)))], [(H, int(rng.integers(1, 9)))]][rng.integers(0, 3)]
    if shape == 0:
        return (clip() + clip()) if rng.random() < 0.8 else []
    core = []
    for _ in range(int(rng.integers(1, 9))):
        core.append((int(rng.choice((M, M, M, I, D, N, S, H, P, EQ, X))), int(rng.integers(0, 30))))
    return clip() + core + clip()


def random_records(seed, n, lengths):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        flag = int(rng.choice((0, 0x10))) | int(rng.choice((0, 0, 0, 0, 0, 0x1, 0x4, 0x100, 0x200, 0x400, 0x800, 0x20)))
        lib = int(rng.choice((0, 0, 1, 1, 2, 2, 3, UNKNOWN)))
        tid = int(rng.choice((-1, 0, 0, 0, 0, 1, 2, 3, 3, 3, len(lengths))))
        length = lengths[tid] if 0 <= tid < len(lengths) else 100
        pos = int(rng.choice((-1, 0, 0, 1, max(0, length - 20), max(0, length - 1), length))) if rng.random() < 0.3 else int(rng.integers(0, max(1, length)))
        out.append((flag, lib, tid, pos, random_cigar(rng)))
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_rule_on_random_records(host_rule, seed):
    lengths = [700, 1, 0, 350]
    # (the sequence of one base gets its two records by hand: chance rarely fits a CIGAR into it)
    records = random_records(seed, 4000, lengths) + [(0, 0, 1, 0, [(S, 3), (M, 1)]), (0x10, 2, 1, 0, [(EQ, 1), (I, 2)])]
    kinds, ivs = host_rule(records, 3, lengths)
    want = PR.brute(records, 3, lengths)
    assert kinds == want["kinds"] and set(kinds) == {PR.IGNORED, PR.COUNTED, PR.OUTSIDE}
    assert ivs == [PR.intervals(r[3], r[4]) if k == PR.COUNTED else [] for r, k in zip(records, kinds)]
    # the host build's intervals as a difference array, summed: the brute force's depth
    for t, n in enumerate(lengths):
        diff = np.zeros(n + 1, np.int64)
        for r, k, iv in zip(records, kinds, ivs):
            if k == PR.COUNTED and r[2] == t:
                for s, e in iv:
                    assert 0 <= s < e <= n
                    diff[s] += 1
                    diff[e] -= 1
        assert (np.cumsum(diff)[:n] == want["depth"][t]).all()
    assert want["counts"]["counted"] > 500 and want["counts"]["outside"] > 500 and want["counts"]["intervals"] > want["counts"]["counted"]
    assert want["per_contig"][1, 3] >= 2 and want["per_contig"][0, 3] > 10 and want["per_contig"][2].tolist() == [0, 0, 0, 0]


def test_runs_of_the_brute_force():
    """The yardstick's own runs: maximal, of depth > 0, and they rebuild the depth."""
    lengths = [60, 0, 1, 40]
    records = [(0, 0, 0, 50, [(M, 10)]), (0, 0, 2, 0, [(M, 1)]), (0, 0, 3, 0, [(M, 5)]), (0, 0, 3, 0, [(M, 3)]), (0, 0, 0, 0, [(M, 2), (D, 2), (M, 2)])]
    want = PR.brute(records, 1, lengths)
    assert [a.tolist() for a in want["runs"]] == [[0, 0, 0, 2, 3, 3], [0, 4, 50, 0, 0, 3], [2, 6, 60, 1, 3, 5], [1, 1, 1, 1, 2, 1]]
    assert want["counts"] == dict(counted=5, outside=0, intervals=6, runs=6)
    assert want["hist"][:3].tolist() == [101 - 20, 17, 3] and want["hist"].sum() == 101


# ---------------------------------------------------------------------- the command line
BASE = ["-i", "in.bam", "-r", "ref.fa"]


@pytest.mark.parametrize("extra,words", [
    (["--depth-bedgraph", "x.bg"], "--depth-bedgraph needs --depth"),
    (["--depth", "--host-decode"], "not with --host-decode"),
    (["--depth", "--gpus", "2"], "--depth cannot be combined with --gpus 2"),
    (["--depth", "--gpus", "2"], "summed across the cards"),
    (["--depth", "-n", "1"], "--depth cannot be combined with -n 1"),
    (["--depth", "-n", "5000"], "--depth cannot be combined with -n 5000"),
    (["--depth", "--rescale-only"], "--depth belongs to the tabulation pass"),
    (["--depth", "--stats-only", "--use-raw-nick-freq", "-d", "."], "--depth belongs to the tabulation pass"),
    (["--depth", "--depth-bedgraph", os.path.join("no", "such", "dir", "x.bg")], "its directory does not exist"),
])
def test_argument_errors(capsys, extra, words):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + extra)
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_bedgraph_that_is_the_input(capsys, tmp_path):
    from mapdamage_amd.main import parse_args
    (tmp_path / "in.bam").write_bytes(b"")
    with pytest.raises(SystemExit) as stop:
        parse_args(["-i", str(tmp_path / "in.bam"), "-r", "ref.fa", "--depth", "--depth-bedgraph", str(tmp_path / "." / "in.bam")])
    assert stop.value.code == 2 and "is the input file" in capsys.readouterr().err


def test_arguments_that_pass(tmp_path):
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--depth"])
    assert o.depth and o.depth_bedgraph is None
    o = parse_args(BASE + ["--depth", "--depth-bedgraph", str(tmp_path / "x.bg"), "--remove-duplicates", "-n", "0.5", "--by-pmd-score",
                           "--merge-libraries", "--min-mapq", "25", "--write-kept", str(tmp_path / "k.bam"), "--chunk-mb", "1"])
    assert o.depth and o.depth_bedgraph == str(tmp_path / "x.bg")
    o = parse_args(BASE)
    assert not o.depth and o.depth_bedgraph is None


# ---------------------------------------------------------------------- the emitters
def test_coverage_text():
    from mapdamage_amd import depth
    names, lengths = ["chr1", "empty", "scaf/1:a"], [3, 0, 7]
    per_contig = np.array([[2, 2, 4, 3], [0, 0, 0, 0], [5, 7, 22, 9]], np.uint64)
    text = depth.coverage_text(names, lengths, per_contig)
    assert text == ("Sequence\tLength\tReads\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth\n"
                    "chr1\t3\t2\t2\t0.666666666666667\t4\t1.33333333333333\t3\n"
                    "empty\t0\t0\t0\tNaN\t0\tNaN\t0\n"
                    "scaf/1:a\t7\t5\t7\t1\t22\t3.14285714285714\t9\n"
                    "*\t10\t7\t9\t0.9\t26\t2.6\t9\n")
    assert text == PR.coverage_text(names, lengths, per_contig)
    # a reference of nothing but empty sequences
    assert depth.coverage_text(["e"], [0], np.zeros((1, 4), np.uint64)).endswith("e\t0\t0\t0\tNaN\t0\tNaN\t0\n*\t0\t0\t0\tNaN\t0\tNaN\t0\n")
    line = depth.log_line(lengths, per_contig, dict(counted=7, outside=3, intervals=9, runs=4))
    assert line == "Depth: 7 records, 26 aligned bases; 9 of 10 reference bases covered (90 %), mean depth 2.6, max 9; 3 records outside their sequence"


def test_histogram_text():
    from mapdamage_amd import depth
    hist = np.zeros(1024, np.uint64)
    hist[[0, 1, 17, 1022, 1023]] = [2**40, 5, 1, 3, 8]
    text = depth.histogram_text(hist)
    assert text == "Depth\tBases\n0\t1099511627776\n1\t5\n17\t1\n1022\t3\n>=1023\t8\n" == PR.histogram_text(hist)
    assert depth.histogram_text(np.zeros(1024, np.uint64)) == "Depth\tBases\n"


def test_bedgraph(tmp_path, monkeypatch):
    from mapdamage_amd import depth
    names = ["chr1", "empty", "scaf/1:a"]
    runs = (np.array([0, 0, 2, 2], np.int32), np.array([0, 5, 0, 2**33], np.int64), np.array([5, 9, 1, 2**33 + 1], np.int64), np.array([1, 4000, 2, 2**32 - 1], np.uint32))
    want = "chr1\t0\t5\t1\nchr1\t5\t9\t4000\nscaf/1:a\t0\t1\t2\nscaf/1:a\t8589934592\t8589934593\t4294967295\n"
    assert b"".join(depth.bedgraph_chunks(names, *runs)).decode() == want == PR.bedgraph_text(names, runs)
    # chunks of three rows and of one: the same text
    assert b"".join(depth.bedgraph_chunks(names, *runs, chunk=3)).decode() == want and len(list(depth.bedgraph_chunks(names, *runs, chunk=1))) == 4
    depth.write_bedgraph(tmp_path / "x.bg", names, *runs)
    assert (tmp_path / "x.bg").read_text() == want and os.listdir(tmp_path) == ["x.bg"]
    depth.write_bedgraph(tmp_path / "none.bg", names, *(a[:0] for a in runs))
    assert (tmp_path / "none.bg").read_text() == ""
    # a failure on the way removes the temporary file and leaves an earlier file alone
    def broken(*args, **kwargs):
        yield b"chr1\t0\t5\t1\n"
        raise OSError("disk full")
    monkeypatch.setattr(depth, "bedgraph_chunks", broken)
    with pytest.raises(OSError):
        depth.write_bedgraph(tmp_path / "x.bg", names, *runs)
    assert sorted(os.listdir(tmp_path)) == ["none.bg", "x.bg"] and (tmp_path / "x.bg").read_text() == want
