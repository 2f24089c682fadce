"""Strata by post-mortem damage score, the parts that need no GPU (``--by-pmd-score``, ``--pmd-thresholds``, ``--pmd-model``):
the table of the terms, the rule itself — the lines the key kernel runs (mapdamage_amd/csrc/mdx_pmd_key.h), compiled for the
host and compared with the restatement of tests/pmd_util.py —, the distance of the fixed point from the formulas' doubles,
the command line's argument errors, the text of ``by_pmd/``, and that the inputs of the GPU tests (tests/test_gpu_pmd.py)
fill every group and enough bins to tell anything."""

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from mapdamage_amd import layout as L
from mapdamage_amd import pmd
from tests import pmd_util as P
from tests.damage_util import resident_reference
from tests.test_gpu_strata import genome5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- the table
def test_the_table_is_the_restatements_bit_for_bit():
    for model in (P.DEFAULT_MODEL, (0.5, 0.0, 0.01), (0.05, 0.2, 0.5)):
        t = pmd.term_table(*model)
        assert t.dtype == np.int32 and t.shape == (2, 256, 95)
        assert t.tolist() == P.restated_table(tuple(model))


def test_spot_values_derived_by_hand():
    t = pmd.term_table()
    fx = lambda v: round(v * 2 ** 24)           # noqa: E731
    # z = 1, no qualities (column 94, eps = 0): D = 0.3 + 0.01 = 0.31, Pm(D) = (1 - D)(1 - pi) = 0.69 x 0.999, Pm(0) = 0.999,
    # so a match is log(0.69) and a mismatch log((1 - 0.68931) / (1 - 0.999)) = log(0.31069 / 0.001)
    assert abs(int(t[0, 0, 94]) - fx(math.log(0.69))) <= 1
    # (0.31069 / 0.001 by hand; the doubles' 1 - 0.999 is 0.001 to 1e-15, a millionth of a unit of the fixed point)
    assert abs(int(t[1, 0, 94]) - fx(math.log(0.31069 / 0.001))) <= 1
    assert 5.7 < t.max() / 2 ** 24 < 5.8 and t.max() == t[1, 0, 94]             # the largest entry, about 5.75 x 2^24
    # z = 1, quality 0: eps = 1/3
    eps, D, pi = 1 / 3, 0.31, 0.001
    pm = lambda D: (1 - D) * (1 - eps) * (1 - pi) + D * eps * (1 - pi) + eps * pi * (1 - D)      # noqa: E731
    assert abs(int(t[0, 0, 0]) - fx(math.log(pm(D) / pm(0)))) <= 1
    assert abs(int(t[1, 0, 0]) - fx(math.log((1 - pm(D)) / (1 - pm(0))))) <= 1
    # quality 93 is not quality 94: eps = 10^-9.3 / 3 moves the mismatch term (1 - Pm(0) = pi + eps (1 - 2 pi) ...) in its
    # seventh digit
    # (d/d eps of the mismatch term at eps = 0 is about -1000 / unit of eps: 1.67e-10 x 1000 x 2^24 = 2.8 units)
    assert t[1, 0, 93] != t[1, 0, 94] and 1 <= int(t[1, 0, 94]) - int(t[1, 0, 93]) <= 4
    # z = 256 against z = 300: positions beyond 256 use D_256 — (1 - p)^255 is 3e-40 at p = 0.3, so D_256 = C to the last bit
    assert abs(int(t[0, 255, 94]) - fx(math.log(0.99))) <= 1
    assert abs(int(t[1, 255, 94]) - fx(math.log(0.01099 / 0.001))) <= 1
    # ... which hides the rule "beyond 256, D_256" at the default model; at p = 0.01 the formula still falls behind z = 256
    # (0.99^255 = 0.077, 0.99^299 = 0.050), and the table's last row is the formula's at 256, not at 300
    slow = pmd.term_table(0.01, 0.0, 0.001)
    at = lambda z: math.log((1 - (1 - 0.01 * 0.99 ** (z - 1)) * 0.999) / (1 - 0.999))          # noqa: E731
    assert abs(int(slow[1, 255, 94]) - fx(at(256))) <= 1 and abs(fx(at(256)) - fx(at(300))) > 1 << 20
    # the terms fall with the distance and a match at the end speaks against damage
    assert (np.diff(t[1, :, 30].astype(np.int64)) <= 0).all() and (t[0] <= 0).all() and (t[1] >= 0).all()


def test_thresholds_names_and_the_fixed_point():
    assert pmd.threshold_fx(3) == 3 << 24 and pmd.threshold_fx(-1.5) == -(3 << 23) and pmd.threshold_fx(0) == 0
    assert pmd.threshold_fx(0.1) == math.ceil(0.1 * 2 ** 24) and pmd.threshold_fx(0.1) * 2 ** -24 >= 0.1 > (pmd.threshold_fx(0.1) - 1) * 2 ** -24
    assert pmd.group_names([3]) == ["<3", ">=3"]
    assert pmd.group_names([-1.5, 0, 2.25, 1e6]) == ["<-1.5", "[-1.5,0)", "[0,2.25)", "[2.25,1e+06)", ">=1e+06"]
    assert pmd.group_names([3]) == P.group_names([3]) and pmd.group_names([0, 1.5, 3]) == P.group_names([0, 1.5, 3])
    for bad in ([], list(range(16)), [1, 1], [2, 1], [0, float("nan")], [1 - 2 ** -30, 1], [1e30], [-1e30, 0], [0, float("inf")]):
        with pytest.raises(ValueError):
            pmd.check_thresholds(bad)
    assert pmd.check_thresholds(range(15)) == [float(k) for k in range(15)]
    for bad in ((0, 0.01, 0.001), (1, 0, 0.001), (0.3, -0.1, 0.001), (0.6, 0.4, 0.001), (0.3, 0.01, 0), (0.3, 0.01, 1)):
        with pytest.raises(ValueError):
            pmd.check_model(*bad)
    assert pmd.check_model(0.5, 0, 0.5) == (0.5, 0.0, 0.5)


# ---------------------------------------------------------------------- the rule, compiled for the host
@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("pmd_key") / "pmd_key_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mapdamage_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pmd_key_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def score(ref, b, packed, single_stranded=False, thresholds=(3.0,), stride=1, with_qual=True, model=P.DEFAULT_MODEL):
        resident, offs = resident_reference(ref)
        seq = np.ascontiguousarray(P.pack4(b.seq) if packed else b.seq)
        terms = np.ascontiguousarray(pmd.term_table(*model))
        fx = np.array([pmd.threshold_fx(t) for t in thresholds], np.int64)
        S, g, bn, nq = np.zeros(b.n, np.int64), np.zeros(b.n, np.uint8), np.zeros(b.n, np.uint8), np.zeros(b.n, np.uint8)
        lib.pmd_scores_host(ctypes.c_int64(b.n), ctypes.c_int64(b.cigar.shape[0]), ctypes.c_int64(b.seq.shape[0]), ptr(b.flag), ptr(b.tid),
                            ptr(b.pos), ptr(b.cigar_off), ptr(b.cigar), ptr(b.seq_off), ptr(seq), ptr(b.qual if with_qual else None),
                            int(packed), ptr(resident), ptr(offs), len(ref.names), int(single_stranded), ptr(terms), len(thresholds),
                            ptr(fx), stride, ptr(S), ptr(g), ptr(bn), ptr(nq))
        return S, g.astype(np.int64), bn.astype(np.int64), nq.astype(bool)
    return score


def test_the_hand_made_records_are_what_they_say():
    ref, b = genome5(), P.hand_batch(genome5(), "kept")
    names = [row[0] for row in P.HAND + P.DEGENERATE]
    ops = lambda i: [int(w) & 15 for w in b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])]]        # noqa: E731
    assert set(ops(names.index("every operation"))) == set(range(9))
    window = lambda i: ref.seqs[int(b.tid[i])][int(b.pos[i]):int(b.pos[i]) + 40].decode()            # noqa: E731
    assert window(names.index("soft-masked reference")).islower()
    assert "N" in window(names.index("reference N run")).upper() and not window(names.index("reference N run")).upper().startswith("N")
    seq = lambda i: b.seq[int(b.seq_off[i]):int(b.seq_off[i + 1])].tobytes().decode()                 # noqa: E731
    assert seq(names.index("lower-case read")).islower()
    assert sorted(len(seq(names.index("%d bases" % n))) for n in (255, 256, 257, 600)) == [255, 256, 257, 600]
    assert {0, 93, 200} <= set(b.qual.tolist()) and (b.flag & 0x10).any()
    S = P.scores(ref, b)
    # a read in lower case pairs with nothing (exact symbols only); the soft-masked reference counts as its upper case
    # (the resident reference is what ref.fetch(...).upper() returns)
    assert S[names.index("lower-case read")] == 0 and S[names.index("soft-masked reference")] != 0
    assert all(S[names.index(row[0])] == 0 for row in P.DEGENERATE) and S[names.index("unmapped")] == 0
    # deamination put in at the ends: the records of the forward strand that show it score high, the rest below zero
    assert S.max() > 5 << 24 and S.min() < -(1 << 24)


@pytest.mark.parametrize("single_stranded", [False, True])
def test_the_rule_equals_the_restatement_on_the_hand_made_records(host_rule, single_stranded):
    ref, b = genome5(), P.hand_batch(genome5(), "kept")
    want = P.scores(ref, b, single_stranded)
    assert (want != P.scores(ref, b, not single_stranded)).any()
    ths = (-1.0, 0.0, 3.0)
    for packed in (False, True):
        for stride in (1, 16, -16, -1):
            S, g, bn, nq = host_rule(ref, b, packed, single_stranded, ths, stride)
            bad = [(P.HAND + P.DEGENERATE)[i][0] for i in np.flatnonzero(S != want)]
            assert not bad, (packed, stride, bad)
            np.testing.assert_array_equal(g, P.groups_of(want, ths))
            np.testing.assert_array_equal(bn, P.bins_of(want))
    # without the quality column every record is scored in column 94
    b0 = P.hand_batch(genome5(), "kept")
    b0.qual = None
    S, _, _, nq = host_rule(ref, b, True, single_stranded, ths, -16, with_qual=False)
    np.testing.assert_array_equal(S, P.scores(ref, b0, single_stranded))
    assert nq.all()
    _, _, _, nq = host_rule(ref, b, True, single_stranded, ths, 1)
    names = [row[0] for row in P.HAND + P.DEGENERATE]
    assert sorted(names[i] for i in np.flatnonzero(nq)) == ["no qualities", "no qualities -", "unmapped"]


@pytest.mark.parametrize("seed,model", [(11, P.DEFAULT_MODEL), (12, (0.45, 0.0, 0.01)), (13, (0.01, 0.0, 0.001))])
def test_the_rule_equals_the_restatement_on_a_seeded_fuzz(host_rule, seed, model):
    """3 000 mixed records of 20 to 300 bases (every kind of operation, clips, both strands, N bases, 3 % dropped), some
    without qualities, some with bytes above 93.  (The third model's terms still change behind z = 256: the records longer
    than that hold the header's clamp to the rule's.)"""
    ref = genome5()
    b = P.synthetic_batch(ref, 3000, seed, 3, len_range=(20, 300))
    rng = np.random.default_rng(seed)
    for i in rng.choice(b.n, 150, replace=False):
        b.qual[int(b.seq_off[i]):int(b.seq_off[i + 1])] = 0xFF
    b.qual[rng.choice(b.qual.shape[0], 2000, replace=False)] = rng.integers(94, 255, 2000).astype(np.uint8)
    ths = (0.0, 1.5, 3.0)
    for single_stranded in (False, True):
        want = P.scores(ref, b, single_stranded, model)
        assert np.count_nonzero(want) > 2800
        for packed, stride in ((False, 1), (True, 16), (True, 7), (True, -16), (False, -16), (True, -5)):
            S, g, bn, _ = host_rule(ref, b, packed, single_stranded, ths, stride, model=model)
            np.testing.assert_array_equal(S, want)
            np.testing.assert_array_equal(g, P.groups_of(want, ths))
            np.testing.assert_array_equal(bn, P.bins_of(want))


def test_groups_and_bins_at_their_edges():
    S = np.array([-(20 << 24) - 1, -(20 << 24), -(20 << 24) + (1 << 23) - 1, -1, 0, (1 << 23) - 1, 1 << 23, (3 << 24) - 1, 3 << 24,
                  (20 << 24) - 1, 20 << 24, 1 << 40], np.int64)
    assert P.bins_of(S).tolist() == [0, 1, 1, 40, 41, 41, 42, 46, 47, 80, 81, 81]
    assert P.groups_of(S, [3]).tolist() == [0] * 8 + [1] * 4
    assert [pmd.bin_edges(b) for b in (0, 1, 41, 80, 81)] == [("-inf", "-20"), ("-20", "-19.5"), ("0", "0.5"), ("19.5", "20"), ("20", "inf")]


# ---------------------------------------------------------------------- the fixed point against the doubles
def test_the_fixed_point_is_within_its_derived_distance_of_the_doubles():
    """S 2^-24 against math.fsum of the formulas' doubles.  Every entry is the double rounded to a multiple of 2^-24: at most
    2^-25 off, so n terms are at most n 2^-25 off in all; fsum rounds the exact sum of the doubles once, the products with
    2^-24 are exact, and 4 ulp of the largest term's binade (4 <= 5.75 < 8) per term bounds what is left generously."""
    ref = genome5()
    b = P.synthetic_batch(ref, 400, 21, 1, len_range=(30, 300))
    worst = 0.0
    for i in range(b.n):
        c0, c1, s0, s1 = int(b.cigar_off[i]), int(b.cigar_off[i + 1]), int(b.seq_off[i]), int(b.seq_off[i + 1])
        ops = [(int(w) & 15, int(w) >> 4) for w in b.cigar[c0:c1]]
        S, doubles = P.score_record(ops, b.seq[s0:s1].tobytes().decode(), b.qual[s0:s1], int(b.flag[i]),
                                    P.window_of(ref, int(b.tid[i]), int(b.pos[i]), ops), want_doubles=True)
        n = len(doubles)
        bound = n * 2.0 ** -25 + n * 4 * math.ulp(4.0)
        err = abs(math.fsum(doubles) - S * 2.0 ** -24)
        assert err <= bound, (i, n, err, bound)
        worst = max(worst, err / bound if n else 0.0)
    assert 0 < worst <= 1


# ---------------------------------------------------------------------- the command line
def _argv(tmp_path, *extra):
    return ["-i", "x.bam", "-r", "x.fa", "-d", str(tmp_path / "out")] + list(extra)


@pytest.mark.parametrize("extra,word", [
    (["--by-pmd-score", "--by-reference"], "exclude each other"),
    (["--by-pmd-score", "--reference-groups", "g.tsv"], "exclude each other"),
    (["--by-pmd-score", "--regions", "p.bed"], "exclude each other"),
    (["--by-pmd-score", "--region-groups", "p.bed"], "exclude each other"),
    (["--by-pmd-score", "--by-terminal-damage"], "exclude each other"),
    (["--by-pmd-score", "--rescale-only"], "--rescale-only"),
    (["--by-pmd-score", "--stats-only", "--fix-nicks"], "--stats-only"),
    (["--by-pmd-score", "-Q", "20"], "quality"),
    (["--by-pmd-score", "--min-basequal", "1"], "--min-basequal"),
    (["--pmd-thresholds", "3"], "need --by-pmd-score"),
    (["--pmd-model", "0.3,0.01,0.001"], "need --by-pmd-score"),
    (["--by-pmd-score", "--pmd-thresholds", "3,1"], "strictly increasing"),
    (["--by-pmd-score", "--pmd-thresholds", "1,1"], "strictly increasing"),
    (["--by-pmd-score", "--pmd-thresholds", ",".join(str(k) for k in range(16))], "1 to 15"),
    (["--by-pmd-score", "--pmd-thresholds", "three"], "--by-pmd-score"),
    (["--by-pmd-score", "--pmd-thresholds", "1e30"], "below 2^38"),
    (["--by-pmd-score", "--pmd-model", "0.3,0.01"], "three numbers"),
    (["--by-pmd-score", "--pmd-model", "0.7,0.3,0.001"], "p + C < 1"),
    (["--by-pmd-score", "--pmd-model", "0.3,0.01,0"], "0 < pi < 1"),
    (["--by-pmd-score", "--pmd-model", "0,0.01,0.001"], "0 < p < 1"),
    (["--by-pmd-score", "--pmd-model", "0.3,-1,0.001"], "0 <= C"),
])
def test_argument_errors(tmp_path, capsys, extra, word):
    from mapdamage_amd.main import main
    assert main(_argv(tmp_path, *extra)) == 1
    assert word in capsys.readouterr().err
    assert not (tmp_path / "out" / "by_pmd").exists()


def test_the_defaults_land_in_the_options(tmp_path):
    from mapdamage_amd.main import PmdScore, build_parser, parse_args, reference_strata
    o = parse_args(_argv(tmp_path))
    assert o.by_pmd_score is False and reference_strata(o, ["chr1"], [10]) is None
    o = parse_args(_argv(tmp_path, "--by-pmd-score"))
    assert reference_strata(o, ["chr1"], [10]) == (["<3", ">=3"], PmdScore((3.0,), (0.3, 0.01, 0.001), False))
    o = parse_args(_argv(tmp_path, "--by-pmd-score", "--pmd-thresholds=-1,0.5,3", "--pmd-model", "0.4,0,0.01", "--single-stranded"))
    assert reference_strata(o, ["chr1"], [10]) == (["<-1", "[-1,0.5)", "[0.5,3)", ">=3"], PmdScore((-1.0, 0.5, 3.0), (0.4, 0.0, 0.01), True))
    helps = {a.option_strings[0]: " ".join((a.help or "").split()) for a in build_parser()._actions if a.option_strings}
    assert "Not a reference option" in helps["--by-pmd-score"] and "--min-basequal" in helps["--by-pmd-score"]


# ---------------------------------------------------------------------- groups.tsv, scores.tsv
def test_groups_tsv_and_scores_tsv_from_hand_made_counts():
    assert pmd.groups_text(["<0", "[0,3)", ">=3"], [7, 0, 12]) == "Index\tGroup\tReads\n0\t<0\t7\n1\t[0,3)\t0\n2\t>=3\t12\n"
    libs = [("Zed", "b"), ("Alpha", "a")]               # (the emitters sort: Alpha first)
    hist = np.zeros((2, 82), np.uint64)
    hist[0, 0], hist[0, 41], hist[0, 81], hist[1, 1], hist[1, 47] = 5, 6, 7, 8, 2 ** 40
    text = pmd.scores_text(libs, hist)
    assert text == P.scores_tsv(libs, hist)
    lines = text.split("\n")
    assert lines[0] == "Sample\tLibrary\tLow\tHigh\tReads" and lines[-1] == "" and len(lines) == 2 + 2 * 82
    assert lines[1] == "Alpha\ta\t-inf\t-20\t0" and lines[2] == "Alpha\ta\t-20\t-19.5\t8" and lines[48] == "Alpha\ta\t3\t3.5\t%d" % 2 ** 40
    assert lines[82] == "Alpha\ta\t20\tinf\t0" and lines[83] == "Zed\tb\t-inf\t-20\t5" and lines[83 + 41] == "Zed\tb\t0\t0.5\t6"
    assert lines[164] == "Zed\tb\t20\tinf\t7"


# ---------------------------------------------------------------------- the inputs of the GPU tests tell something
def test_the_gpu_tests_inputs_fill_every_group_and_ten_bins():
    from tests import test_gpu_pmd as G
    for name, (ref, b, nlib, ths, single_stranded) in G.inputs().items():
        S = P.scores(ref, b, single_stranded)
        keep = ((b.flag & 0xF04) == 0) & (b.lib < nlib)
        per_group = np.bincount(P.groups_of(S, ths)[keep], minlength=len(ths) + 1)
        assert per_group.min() >= 1, (name, per_group)
        assert np.count_nonzero(P.histogram(b, S, nlib).sum(axis=0)) >= 10, name
