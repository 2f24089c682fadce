"""--depth-regions on the host: the four emitters of mapdamage_amd/depth.py against hand-written text, the thresholds, the
brute force of tests/depth_regions_rule.py on a case small enough to check by eye, and the command line's argument errors.  The
device pass and the run's files: tests/test_gpu_depth_regions.py."""

import numpy as np
import pytest

from tests import depth_regions_rule as RR

GROUPS = ["bait A", "empty", "*"]


def hist_of(pairs, n_groups=3):
    h = np.zeros((n_groups, 1024), np.uint64)
    for g, d, n in pairs:
        h[g, d] = n
    return h


# ---------------------------------------------------------------------- the emitters
def test_coverage_text():
    from mapdamage_amd import depth
    per_group = np.array([[30, 20, 45, 7], [0, 0, 0, 0], [2**33, 3, 2**40, 5000]], np.uint64)
    assert depth.region_coverage_text(GROUPS, [2, 0, 0], per_group) == (
        "Index\tGroup\tRegions\tBases\tCovered\tBreadth\tAlignedBases\tMeanDepth\tMaxDepth\n"
        "0\tbait A\t2\t30\t20\t0.666666666666667\t45\t1.5\t7\n"
        "1\tempty\t0\t0\t0\tNaN\t0\tNaN\t0\n"
        "2\t*\t0\t8589934592\t3\t3.49245965480804e-10\t1099511627776\t128\t5000\n")
    assert depth.region_coverage_text(GROUPS, [2, 0, 0], per_group) == RR.coverage_text(GROUPS, [0, 0], per_group)


def test_histogram_text():
    from mapdamage_amd import depth
    h = hist_of([(0, 0, 10), (0, 3, 19), (0, 1023, 1), (2, 0, 2**40), (2, 1022, 4), (2, 1023, 6)])
    text = depth.region_histogram_text(GROUPS, h)
    assert text == ("Index\tGroup\tDepth\tBases\n"
                    "0\tbait A\t0\t10\n0\tbait A\t3\t19\n0\tbait A\t>=1023\t1\n"
                    "2\t*\t0\t1099511627776\n2\t*\t1022\t4\n2\t*\t>=1023\t6\n")
    assert text == RR.histogram_text(GROUPS, h)
    # a group's lines sum to its bases
    assert sum(int(line.split("\t")[3]) for line in text.splitlines()[1:] if line.startswith("0\t")) == 30


def test_thresholds_from_a_histogram_whose_last_bin_is_not_empty():
    from mapdamage_amd import depth
    h = hist_of([(0, 0, 10), (0, 1, 4), (0, 5, 5), (0, 1022, 8), (0, 1023, 3), (2, 0, 7)])
    per_group = np.array([[30, 20, 0, 0], [0, 0, 0, 0], [7, 0, 0, 0]], np.uint64)
    assert depth.bases_at_least(h[0], [1, 2, 5, 6, 1022]) == [20, 16, 16, 11, 11]
    text = depth.region_thresholds_text(GROUPS, per_group, h, [1, 6, 1022])
    assert text == ("Index\tGroup\tThreshold\tBases\tFraction\n"
                    "0\tbait A\t1\t20\t0.666666666666667\n0\tbait A\t6\t11\t0.366666666666667\n0\tbait A\t1022\t11\t0.366666666666667\n"
                    "1\tempty\t1\t0\tNaN\n1\tempty\t6\t0\tNaN\n1\tempty\t1022\t0\tNaN\n"
                    "2\t*\t1\t0\t0\n2\t*\t6\t0\t0\n2\t*\t1022\t0\t0\n")
    assert text == RR.thresholds_text(GROUPS, per_group, h, [1, 6, 1022])


REGIONS = dict(names=["chr1", "none", "scaf/1:a"], iv_off=[0, 2, 2, 5], iv_start=[0, 10, 0, 1, 2**31 - 8], iv_end=[3, 17, 1, 4, 2**31 - 1],
               iv_group=[0, 1, 1, 0, 1])
PER_INTERVAL = np.array([[2, 4, 0, 3], [7, 7 * 2**33, 2**33, 2**33], [0, 0, 0, 0], [3, 5000, 1, 4998], [1, 1, 0, 1]], np.uint64)
REGIONS_TEXT = ("chr1\t0\t3\tbait A\t2\t0.666666666666667\t4\t1.33333333333333\t0\t3\n"
                "chr1\t10\t17\tempty\t7\t1\t60129542144\t8589934592\t8589934592\t8589934592\n"
                "scaf/1:a\t0\t1\tempty\t0\t0\t0\t0\t0\t0\n"
                "scaf/1:a\t1\t4\tbait A\t3\t1\t5000\t1666.66666666667\t1\t4998\n"
                "scaf/1:a\t2147483640\t2147483647\tempty\t1\t0.142857142857143\t1\t0.142857142857143\t0\t1\n")


@pytest.mark.parametrize("chunk", [1, 2, 3, 5, 1 << 18])
def test_regions_depth_chunks(chunk):
    """Every chunk size gives the same bytes: a boundary after every row, inside a sequence, at the last row."""
    from mapdamage_amd import depth
    r = REGIONS
    parts = list(depth.regions_depth_chunks(r["names"], GROUPS, r["iv_off"], r["iv_start"], r["iv_end"], r["iv_group"], PER_INTERVAL, chunk=chunk))
    assert len(parts) == -(-5 // chunk) and b"".join(parts).decode() == REGIONS_TEXT
    assert depth.REGIONS_DEPTH_HEADER + REGIONS_TEXT == RR.regions_depth_text(r["names"], GROUPS, r["iv_off"], r["iv_start"], r["iv_end"],
                                                                             r["iv_group"], PER_INTERVAL)
    assert list(depth.regions_depth_chunks(r["names"], GROUPS, [0, 0, 0, 0], [], [], [], np.zeros((0, 4), np.uint64), chunk=chunk)) == []


def test_write_region_files(tmp_path):
    from mapdamage_amd import depth
    from mapdamage_amd.tables import Regions
    r = REGIONS
    regions = Regions(np.array(r["iv_off"], np.int64), np.array(r["iv_start"], np.int32), np.array(r["iv_end"], np.int32),
                      np.array(r["iv_group"], np.int32), [20, 5, 2**31 - 1])
    per_group = np.array([[6, 5, 5004, 4998], [15, 8, 7 * 2**33 + 1, 2**33], [2**31 + 3, 0, 0, 0]], np.uint64)
    h = hist_of([(0, 0, 1), (0, 3, 5), (1, 0, 7), (1, 1023, 8), (2, 0, 2**31 + 3)])
    depth.write_region_files(tmp_path, r["names"], GROUPS, regions, (PER_INTERVAL, per_group, h), [1, 5])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["coverage.tsv", "depth_histogram.tsv", "depth_thresholds.tsv", "regions_depth.tsv"]
    assert (tmp_path / "regions_depth.tsv").read_text() == depth.REGIONS_DEPTH_HEADER + REGIONS_TEXT
    assert (tmp_path / "coverage.tsv").read_text().splitlines()[1] == "0\tbait A\t2\t6\t5\t0.833333333333333\t5004\t834\t4998"
    assert (tmp_path / "depth_thresholds.tsv").read_text().splitlines()[3:5] == ["1\tempty\t1\t8\t0.533333333333333", "1\tempty\t5\t8\t0.533333333333333"]
    assert (tmp_path / "depth_histogram.tsv").read_text() == RR.histogram_text(GROUPS, h)


def test_log_line():
    from mapdamage_amd import depth
    per_group = np.array([[30, 20, 45, 7], [10, 10, 15, 3], [100, 3, 25, 5000]], np.uint64)
    assert depth.region_log_line(per_group) == "Depth on target: 30 of 40 target bases covered (75 %), mean depth 1.5 on target, 0.25 off target"
    assert depth.region_log_line(np.array([[0, 0, 0, 0], [0, 0, 0, 0]], np.uint64)) == (
        "Depth on target: 0 of 0 target bases covered (NaN %), mean depth NaN on target, NaN off target")


# ---------------------------------------------------------------------- the brute force itself
def test_the_brute_force_by_eye():
    depth = [np.array([0, 2, 2, 1, 0, 0, 5, 2000]), np.zeros(0, np.int64), np.array([3, 0])]
    per_interval, per_group, group_hist = RR.brute(depth, [0, 2, 2, 3], [1, 3, 1], [3, 7, 2], [0, 1, 0], 3)
    assert per_interval.tolist() == [[2, 4, 2, 2], [2, 6, 0, 5], [0, 0, 0, 0]]
    assert per_group.tolist() == [[3, 2, 4, 2], [4, 2, 6, 5], [3, 2, 2003, 2000]]
    assert group_hist.sum(axis=1).tolist() == [3, 4, 3] and group_hist[2, 1023] == 1 and group_hist[2, 3] == 1 and group_hist[2, 0] == 1
    assert group_hist[0, 2] == 2 and group_hist[0, 0] == 1 and group_hist[1, [0, 1, 5]].tolist() == [2, 1, 1]


# ---------------------------------------------------------------------- the command line
BASE = ["-i", "in.bam", "-r", "ref.fa"]
ON = ["--depth", "--regions", "x.bed", "--depth-regions"]


@pytest.mark.parametrize("extra,words", [
    (["--depth-regions", "--regions", "x.bed"], "--depth-regions needs --depth"),
    (["--depth-regions", "--depth"], "--depth-regions needs --regions or --region-groups"),
    (["--depth-regions", "--depth", "--by-reference"], "--depth-regions needs --regions or --region-groups"),
    (["--depth-thresholds", "1,5", "--depth", "--regions", "x.bed"], "--depth-thresholds needs --depth-regions"),
    (["--depth-thresholds", "1,5"], "--depth-thresholds needs --depth-regions"),
    (ON + ["--depth-thresholds", "1,x"], "a comma-separated list of integers"),
    (ON + ["--depth-thresholds", ""], "a comma-separated list of integers"),
    (ON + ["--depth-thresholds", "1.5"], "a comma-separated list of integers"),
    (ON + ["--depth-thresholds", "0,5"], "every threshold lies in 1..1022"),
    (ON + ["--depth-thresholds", "5,1023"], "every threshold lies in 1..1022"),
    (ON + ["--depth-thresholds", "5,5"], "must increase strictly"),
    (ON + ["--depth-thresholds", "10,5"], "must increase strictly"),
    (ON + ["--depth-thresholds", ",".join(str(t) for t in range(1, 34))], "at most 32"),
    # every restriction of --depth stands
    (ON + ["--host-decode"], "not with --host-decode"),
    (ON + ["--gpus", "2"], "--depth cannot be combined with --gpus 2"),
    (ON + ["-n", "5000"], "--depth cannot be combined with -n 5000"),
])
def test_argument_errors(capsys, extra, words):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as stop:
        parse_args(BASE + extra)
    assert stop.value.code == 2
    assert words in capsys.readouterr().err


def test_arguments_that_pass():
    from mapdamage_amd.main import parse_args
    o = parse_args(BASE + ["--depth"])
    assert o.depth and o.depth_regions is False and o.depth_thresholds is None
    o = parse_args(BASE + ["--depth", "--regions", "x.bed"])
    assert o.depth_regions is False and o.depth_thresholds is None
    o = parse_args(BASE + ON)
    assert o.depth_regions is True and o.depth_thresholds == [1, 5, 10, 20]
    o = parse_args(BASE + ["--depth", "--region-groups", "x.bed", "--depth-regions", "--only-regions", "--depth-thresholds",
                           ",".join(str(t) for t in range(991, 1023))])
    assert o.depth_regions is True and o.depth_thresholds == list(range(991, 1023))
