"""--remove-duplicates, the parts that need no GPU: the rule (mapdamage_amd/csrc/mdx_dup_key.h compiled for the host, against
the brute force of tests/dup_rule.py), the set of signatures (csrc/mdx_dup_table.h single-threaded, as the stand-alone program
tests/native/dup_table_check.cpp, once more under AddressSanitizer and UBSan, against a Python dict), and the command line's
argument errors.  The device stage: tests/test_gpu_remove_duplicates.py."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import dup_rule as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8


# ---------------------------------------------------------------------- the rule
@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("dup_key") / "dup_key_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "dup_key_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))

    def rule(records, n_libraries, ends, cigar_off=None, n_cigar=None):
        flag, lib_, tid, pos, off, cigar = DR.columns(records)
        off = off if cigar_off is None else np.asarray(cigar_off, np.uint32)
        n = len(records)
        kind, sig = np.zeros(n, np.int32), np.zeros(2 * n, np.uint64)
        cigar = np.concatenate([cigar, np.zeros(1, np.uint32)])         # (never empty)
        lib.dup_key_host(ctypes.c_int64(n), ctypes.c_int64(len(cigar) - 1 if n_cigar is None else n_cigar), *(ctypes.c_void_p(a.ctypes.data)
                         for a in (flag, lib_, tid, pos, off, cigar)), ctypes.c_int(n_libraries), ctypes.c_int(DR_ENDS[ends]),
                         ctypes.c_void_p(kind.ctypes.data), ctypes.c_void_p(sig.ctypes.data))
        return kind, [(int(sig[2 * i]), int(sig[2 * i + 1])) for i in range(n)]
    return rule


DR_ENDS = {"both": 0, "5p": 1}


def random_cigar(rng):
    shape = rng.integers(0, 8)
    lead = [[], [(S, int(rng.integers(1, 9)))], [(H, int(rng.integers(1, 9)))], [(H, int(rng.integers(1, 5))), (S, int(rng.integers(1, 5)))]][rng.integers(0, 4)]
    trail = [[], [(S, int(rng.integers(1, 9)))], [(H, int(rng.integers(1, 9)))], [(S, int(rng.integers(1, 5))), (H, int(rng.integers(1, 5)))]][rng.integers(0, 4)]
    if shape == 0:
        return (lead + trail) if rng.random() < 0.8 else []            # clips only, or no CIGAR at all
    core = [(M, int(rng.integers(1, 40)))]
    for _ in range(int(rng.integers(0, 4))):
        core.append((int(rng.choice((I, D, N, EQ, X, M))), int(rng.integers(1, 12))))
    core.append((int(rng.choice((M, EQ, X))), int(rng.integers(1, 40))))
    return lead + core + trail


def random_records(seed, n, n_libraries=3):
    """A few positions, so that records collide by chance, with every shape of CIGAR, both strands, every kind of record."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        flag = int(rng.choice((0, 0x10))) | int(rng.choice((0, 0, 0, 0x1, 0x4, 0x100, 0x200, 0x400, 0x800, 0x20, 0x40)))
        lib = int(rng.choice((0, 1, 2, 2, 3, 0xFFFF)))                # (3 and 0xFFFF: not a library the context knows)
        tid = int(rng.choice((-1, 0, 0, 1, 1, 2)))
        pos = int(rng.choice((-1, 0, 0, 1, 5, 7, 100, 101, 102)))
        # (half of them from a few shapes, so that molecules meet by chance — `5S15M` at 5 and `20M` at 0 among them)
        out.append((flag, lib, tid, pos, MENU[rng.integers(0, len(MENU))] if rng.random() < 0.5 else random_cigar(rng)))
    return out


MENU = [[(M, 20)], [(S, 5), (M, 15)], [(H, 5), (M, 15)], [(M, 15), (S, 5)], [(M, 10), (D, 5), (M, 5)], [(M, 10), (I, 5), (M, 10)],
        [(H, 1), (S, 4), (EQ, 10), (X, 5)], [(M, 21)], [(S, 1), (M, 19)], [(M, 18), (S, 1), (H, 1)]]


def same_partition(kinds, sigs, records, n_libraries, ends):
    """The host build calls two records copies exactly where the brute force does, and examines the same ones."""
    want = [DR.signature(*r, n_libraries, ends) for r in records]
    assert kinds.tolist() == [k for k, _ in want]
    first, first_want = {}, {}
    for i, ((k, s), g) in enumerate(zip(want, sigs)):
        if k == DR.EXAMINED:
            assert g[0] != 2**64 - 1
            assert first.setdefault(g, i) == first_want.setdefault(s, i), (i, records[i])


@pytest.mark.parametrize("ends", ["both", "5p"])
@pytest.mark.parametrize("seed", [1, 2])
def test_rule_on_random_records(host_rule, seed, ends):
    records = random_records(seed, 4000)
    kinds, sigs = host_rule(records, 3, ends)
    same_partition(kinds, sigs, records, 3, ends)
    assert {DR.IGNORED, DR.EXAMINED, DR.PAIRED, DR.OTHER} == set(kinds.tolist())
    dup = DR.brute(records, 3, ends)[0]
    assert 100 < dup.sum() < len(records) - 100


def test_rule_directed_pairs(host_rule):
    p = 1000
    base = (0, 0, 1, p, [(M, 100)])
    collide = [(0, 0, 1, p + 5, [(S, 5), (M, 95)]), (0, 0, 1, p + 7, [(H, 3), (S, 4), (M, 93)]), (0, 0, 1, p, [(M, 90), (S, 10)]),
               (0, 0, 1, p, [(M, 40), (D, 10), (M, 50)]), (0, 0, 1, p, [(EQ, 50), (X, 1), (M, 20), (I, 7), (N, 9), (M, 20)]),
               (0x20, 0, 1, p, [(M, 100)])]
    differ = [(0x10, 0, 1, p, [(M, 100)]), (0, 1, 1, p, [(M, 100)]), (0, 0, 0, p, [(M, 100)]), (0, 0, 1, p, [(M, 99)]),
              (0, 0, 1, p + 1, [(M, 99)]), (0, 0, 1, p, [(M, 100), (S, 1)])]
    for other in collide + differ:
        (ka, kb), (sa, sb) = host_rule([base, other], 2, "both")
        assert ka == kb == DR.EXAMINED and (sa == sb) == (other in collide), other
        assert (DR.signature(*base, 2)[1] == DR.signature(*other, 2)[1]) == (other in collide)
    # 5p: the same 5' end with another 3' end collides — forwards the left end, on the reverse strand the right one
    for a, b, same in [((0, 0, 1, p, [(M, 100)]), (0, 0, 1, p, [(M, 60)]), True), ((0, 0, 1, p, [(M, 100)]), (0, 0, 1, p + 40, [(M, 60)]), False),
                       ((0x10, 0, 1, p, [(M, 100)]), (0x10, 0, 1, p + 40, [(M, 60)]), True), ((0x10, 0, 1, p, [(M, 100)]), (0x10, 0, 1, p, [(M, 60)]), False),
                       ((0x10, 0, 1, p, [(M, 100)]), (0x10, 0, 1, p + 40, [(M, 50), (S, 10)]), True),
                       # (a forward record's left end is no reverse record's right end, whatever the numbers)
                       ((0, 0, 1, p, [(M, 1)]), (0x10, 0, 1, p, [(M, 1)]), False)]:
        (ka, kb), (sa, sb) = host_rule([a, b], 2, "5p")
        assert ka == kb == DR.EXAMINED and (sa == sb) == same, (a, b)
        assert (DR.signature(*a, 2, "5p")[1] == DR.signature(*b, 2, "5p")[1]) == same
        assert host_rule([a, b], 2, "both")[1][0] != host_rule([a, b], 2, "both")[1][1]


def test_rule_at_the_edges(host_rule):
    big = 2**28 - 1                        # the longest operation BAM can hold
    records = [
        (0, 0, 0, 0, [(S, 5), (M, 10)]),                                   # left = -5
        (0, 0, 0, 0, [(H, 2), (S, 3), (M, 10)]),                           # the same molecule
        (0, 0, 0, 0, [(H, big)] * 8 + [(H, 8), (M, 10)]),                  # left = -2^31 exactly: fits
        (0, 0, 0, 0, [(H, big)] * 8 + [(H, 9), (M, 10)]),                  # one below: not examined
        (0, 0, 0, 2**31 - 1, [(M, 1), (S, big)] + [(H, big)] * 7 + [(H, 8)]),      # right = 2^31 - 1 + 8 (2^28 - 1) + 8 = 2^32 - 1
        (0, 0, 0, 2**31 - 1, [(M, 1), (S, big)] + [(H, big)] * 7 + [(H, 9)]),      # one above: not examined
        (0, 0, 0, 2**31 - 1, [(M, 1)]),
        (0, 0, 0, 7, [(S, 4), (H, 4)]),                                    # clips only
        (0, 0, 0, 7, []),                                                  # no CIGAR
        (0, 0, 0, 7, [(I, 4)]),                                            # nothing on the reference
        (0, 0, 0, 7, [(N, 4)]),                                            # N alone consumes the reference
        (0, 0, -1, 7, [(M, 4)]), (0, 0, 0, -1, [(M, 4)]),
        (0, 0xFFFF, 0, 7, [(M, 4)]), (0, 2, 0, 7, [(M, 4)]),               # no library of the context's two
        (0x1, 0, 0, 7, [(M, 4)]), (0x401, 0, 0, 7, [(M, 4)]),              # paired; paired and dropped: the filter comes first
    ]
    for ends in ("both", "5p"):
        kinds, sigs = host_rule(records, 2, ends)
        same_partition(kinds, sigs, records, 2, ends)
        E, O, P, G = DR.EXAMINED, DR.OTHER, DR.PAIRED, DR.IGNORED
        assert kinds.tolist() == [E, E, E, O, E, O, E, O, O, O, E, O, O, G, G, P, G]
        assert sigs[0] == sigs[1] and sigs[2] != sigs[0]
    # offsets beyond the CIGAR column are clamped to it: the record has the operations that are there, or none
    two = [(0, 0, 0, 10, [(M, 5)]), (0, 0, 0, 10, [(M, 5), (S, 3)])]
    kinds, sigs = host_rule(two, 1, "both", cigar_off=[0, 1, 9], n_cigar=2)
    assert kinds.tolist() == [DR.EXAMINED, DR.EXAMINED] and sigs[0] == sigs[1]          # (M 5 alone: the S lies beyond)
    kinds, _ = host_rule(two, 1, "both", cigar_off=[5, 7, 9], n_cigar=3)
    assert kinds.tolist() == [DR.OTHER, DR.OTHER]


# ---------------------------------------------------------------------- the table
def table_program(tmp_path_factory, flags, name):
    exe = tmp_path_factory.mktemp(name) / "dup_table_check"
    subprocess.check_call(["g++", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "native", "dup_table_check.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan-ubsan"])
def table_exe(request, tmp_path_factory):
    return table_program(tmp_path_factory, request.param, "dup_table")


def drive(exe, slots, mode, batches):
    """``batches``: [(signatures, order)], order 0, 1 or a permutation -> the program's (duplicate bits, slots, growths, {ordinal: count})."""
    text = ["T %d %d" % (slots, mode)]
    for sigs, order in batches:
        text.append("B %d %d" % (len(sigs), order if isinstance(order, int) else 2))
        text += ["%x %x" % s for s in sigs]
        if not isinstance(order, int):
            text.append(" ".join(str(int(j)) for j in order))
    text.append("E")
    out = subprocess.run([exe], input=("\n".join(text) + "\n").encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
    assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
    lines = out.stdout.decode().split("\n")
    assert lines[-2] == "OK"
    bits = "".join(line[2:] for line in lines if line.startswith("D "))
    (_, n_slots, growths), = [line.split() for line in lines if line.startswith("S ")]
    return bits, int(n_slots), int(growths), {int(line.split()[1]): int(line.split()[2]) for line in lines if line.startswith("M ")}


def by_dict(batches):
    first, count, bits = {}, {}, []
    for i, s in enumerate(s for sigs, _ in batches for s in sigs):
        bits.append("1" if s in first else "0")
        first.setdefault(s, i)
        count[first[s]] = count.get(first[s], 0) + 1
    return "".join(bits), count


@pytest.mark.parametrize("mode", [0, 1], ids=["hashed", "one chain"])
def test_table_against_a_dict(table_exe, mode):
    rng = np.random.default_rng(5 + mode)
    n = 3000 if mode == 0 else 600                  # (one chain: every insert walks all the molecules in front)
    keys = [(int(rng.integers(0, 4)) << 32 | int(rng.integers(0, 3)) << 16, int(rng.integers(0, 8)) << 32 | int(rng.integers(0, 8))) for _ in range(n)]
    cuts = sorted(rng.choice(np.arange(1, n), 9, replace=False).tolist())
    batches = []
    for k, (lo, hi) in enumerate(zip([0] + cuts, cuts + [n])):
        batches.append((keys[lo:hi], [0, 1, rng.permutation(hi - lo)][k % 3]))
    bits, slots, growths, molecules = drive(table_exe, 8, mode, batches)
    want_bits, want = by_dict(batches)
    assert bits == want_bits and molecules == want
    assert 100 < bits.count("1") < n - 100
    assert slots >= 2 * n and slots & (slots - 1) == 0 and growths >= 3           # from 8 slots


def test_table_equal_keys_in_descending_order(table_exe):
    """All records of a batch are one molecule and go in last first: each insert finds a larger ordinal in the slot and takes
    it over; the first in file order is the one that stays."""
    batches = [([(7, 9)] * 500, 1), ([(7, 9)] * 300 + [(7, 10)] * 5, 1)]
    bits, _, growths, molecules = drive(table_exe, 8, 0, batches)
    assert bits == "0" + "1" * 799 + "0" + "1" * 4 and molecules == {0: 800, 800: 5} and growths == 2


# ---------------------------------------------------------------------- the command line
BASE = ["-i", "in.bam", "-r", "ref.fa"]


@pytest.mark.parametrize("extra,words", [
    (["--duplicate-ends", "5p"], "--duplicate-ends needs --remove-duplicates"),
    (["--remove-duplicates", "--host-decode"], "not with --host-decode"),
    (["--remove-duplicates", "--gpus", "2"], "--remove-duplicates cannot be combined with --gpus 2"),
    (["--remove-duplicates", "-n", "1"], "--remove-duplicates cannot be combined with -n 1"),
    (["--remove-duplicates", "-n", "5000"], "--remove-duplicates cannot be combined with -n 5000"),
    (["--remove-duplicates", "--rescale-only"], "--remove-duplicates belongs to the tabulation pass"),
    (["--remove-duplicates", "--stats-only", "--use-raw-nick-freq", "-d", "."], "--remove-duplicates belongs to the tabulation pass"),
    (["--remove-duplicates", "--duplicate-ends", "3p"], "invalid choice"),
])
def test_argument_errors(capsys, extra, words):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + extra)
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_arguments_that_pass():
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--remove-duplicates"])
    assert o.remove_duplicates and o.duplicate_ends == "both"
    o = parse_args(BASE + ["--remove-duplicates", "--duplicate-ends", "5p", "-n", "0.5", "--by-pmd-score", "--merge-libraries", "--min-mapq", "25"])
    assert o.duplicate_ends == "5p"
    o = parse_args(BASE)
    assert not o.remove_duplicates and o.duplicate_ends is None
