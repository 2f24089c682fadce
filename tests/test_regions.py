"""Regions on the host: the BED parser of ``--regions`` / ``--region-groups``, ``groups.tsv`` and the argument errors
(the device side: tests/test_gpu_regions.py)."""

import numpy as np
import pytest

from tests import regions_util as R

REFS = ["chr1", "chr2", "chrM", "sc:1/*", "empty"]
LENS = [9000, 5000, 3000, 2500, 100]


def parse(text, named=True, refs=REFS, lens=LENS):
    from mapdamage_amd.tables import parse_regions
    names, off, start, end, group = parse_regions(text, refs, lens, named)
    assert off.dtype == np.int64 and start.dtype == end.dtype == group.dtype == np.int32
    return names, off.tolist(), start.tolist(), end.tolist(), group.tolist()


def test_groups_are_numbered_by_first_appearance_and_the_rest_is_last():
    names, off, start, end, group = parse("chr2\t10\t20\tpanel_b\nchr1\t5\t9\tpanel_a\tand\tmore columns\nchr2\t40\t41\tpanel_b\n"
                                          "sc:1/*\t0\t2500\tpanel_c\n")
    assert names == ["panel_b", "panel_a", "panel_c", "*"]
    assert off == [0, 1, 3, 3, 4, 4]                 # chrM and 'empty' have no regions
    assert (start, end, group) == ([5, 10, 40, 0], [9, 20, 41, 2500], [1, 0, 0, 2])


def test_unnamed_regions_are_one_group():
    names, off, start, end, group = parse("chr1\t100\t200\tignored\nchrM\t0\t1\n", named=False)
    assert names == ["regions", "*"] and off == [0, 1, 1, 2, 2, 2]
    assert (start, end, group) == ([100, 0], [200, 1], [0, 0])
    # no region at all: '*' is still there
    assert parse("# nothing\n", named=False) == (["regions", "*"], [0] * 6, [], [], [])
    assert parse("", named=True)[0] == ["*"]


def test_same_group_regions_merge_when_they_overlap_or_abut_and_input_order_does_not_matter():
    text = ("chr1\t300\t400\ta\n"
            "chr1\t100\t200\ta\n"
            "chr1\t200\t250\ta\n"        # abuts the one before
            "chr1\t120\t130\ta\n"        # inside it
            "chr1\t390\t450\ta\n"        # overlaps [300, 400)
            "chr1\t450\t460\tb\n"        # abuts, another group: stays
            "chr1\t251\t260\ta\n"        # one base of gap: stays
            "chr2\t7\t8\tb\n")
    names, off, start, end, group = parse(text)
    assert names == ["a", "b", "*"] and off == [0, 4, 5, 5, 5, 5]
    assert start == [100, 251, 300, 450, 7] and end == [250, 260, 450, 460, 8] and group == [0, 0, 0, 1, 1]
    lines = text.splitlines()
    for seed in range(5):
        shuffled = [lines[i] for i in np.random.default_rng(seed).permutation(len(lines))]
        got = parse("\n".join(shuffled) + "\n")
        order = [got[0].index(n) for n in names]                     # (the numbering follows the order of appearance)
        assert got[1:4] == (off, start, end) and [order.index(g) for g in got[4]] == group


def test_skipped_lines_and_line_ends():
    text = "#comment\ntrack name=x\nbrowser position chr1:1-2\n\n   \nchr1\t1\t2\tg\r\nchr2\t3\t4\tg"
    assert parse(text) == (["g", "*"], [0, 1, 2, 2, 2, 2], [1, 3], [2, 4], [0, 0])
    # a sequence may be named like the skipped words' prefix
    assert parse("tracker\t1\t2\tg\n", refs=["tracker"], lens=[10])[2] == [1]


def test_the_output_is_sorted_and_disjoint_for_the_grid_regions():
    regs = R.grid_regions()
    names, off, start, end, group = parse(R.bed_text(regs, REFS, R.GRID_GROUPS), lens=list(R.GRID_LENGTHS))
    assert set(names) == set(R.GRID_GROUPS) and names[-1] == "*"
    assert off[2] == off[3]                                          # chrM: none
    for t in range(5):
        s, e = start[off[t]:off[t + 1]], end[off[t]:off[t + 1]]
        assert all(a < b for a, b in zip(s, e)) and all(b <= c for b, c in zip(e[:-1], s[1:]))
    # (grid_regions lists no two abutting regions of one group: nothing to merge)
    assert sorted(zip(start, end)) == sorted((s, e) for _, s, e, _ in regs)


@pytest.mark.parametrize("text,words", [
    ("chr1\t1\t2\tg\nchr1\t5\n", ["line 2"]),                                      # fewer than three columns
    ("chr1 1 2 g\n", ["line 1"]),                                                  # (blanks are no tabs)
    ("chr1\t1\t2\tg\n\nchr1\tx\t9\tg\n", ["line 3", "'x'"]),                       # coordinates
    ("chr1\t1.5\t9\tg\n", ["line 1", "'1.5'"]),
    ("chr1\t9\t9\tg\n", ["line 1", "[9, 9)"]),                                     # start >= end
    ("chr1\t10\t9\tg\n", ["line 1"]),
    ("chr1\t-1\t9\tg\n", ["line 1"]),
    ("chr1\t1\t2\tg\nchr2\t4990\t5001\tg\n", ["line 2", "5001", "5000", "chr2"]),  # beyond the sequence
    ("#c\nchrQ\t1\t2\tg\n", ["line 2", "chrQ"]),                                   # not in the header
    ("chr1\t1\t2\t*\n", ["line 1", "'*'"]),                                        # the rest's name
    ("chr1\t1\t2\tg\nchr1\t5\t6\n", ["line 2", "column 4"]),                       # no name
    ("chr1\t1\t2\tg\nchr1\t5\t6\t\n", ["line 2", "column 4"]),
])
def test_errors_name_the_line(text, words):
    with pytest.raises(ValueError) as err:
        parse(text)
    for w in words:
        assert w in str(err.value), (w, str(err.value))


def test_overlapping_regions_of_different_groups_name_both_lines():
    with pytest.raises(ValueError) as err:
        parse("chr2\t1\t2\tb\nchr1\t100\t200\ta\n# c\nchr1\t300\t310\ta\nchr1\t199\t250\tb\n")
    assert "lines 2 and 5" in str(err.value) and "'a'" in str(err.value) and "'b'" in str(err.value)
    # ... the two that overlap, not the ones merged with them
    with pytest.raises(ValueError) as err:
        parse("chr1\t100\t200\ta\nchr1\t150\t400\ta\nchr1\t120\t130\tb\n")
    assert "lines 1 and 3" in str(err.value)
    with pytest.raises(ValueError) as err:
        parse("chr1\t350\t360\tb\nchr1\t100\t200\ta\nchr1\t150\t400\ta\n")
    assert "lines 1 and 3" in str(err.value)
    # the same regions without names: one group, merged
    assert parse("chr1\t100\t200\ta\nchr1\t199\t250\tb\n", named=False)[2:4] == ([100], [250])
    # abutting is no overlap
    assert parse("chr1\t100\t200\ta\nchr1\t200\t250\tb\n")[2:4] == ([100, 200], [200, 250])


def test_groups_tsv_counts_regions_and_bases_after_merging():
    from mapdamage_amd.tables import parse_regions, region_groups_text
    text = ("chr1\t100\t200\ta\nchr1\t200\t250\ta\nchr1\t120\t130\ta\nchr1\t400\t401\tb\nchr2\t0\t5000\ta\nchrM\t5\t10\tc\n"
            "chrM\t8\t30\tc\n")
    names, off, start, end, group = parse_regions(text, REFS, LENS, True)
    got = region_groups_text(names, start, end, group, LENS, [7, 0, 11, 12345])
    total = sum(LENS)
    assert got == ("Index\tGroup\tRegions\tBases\tReads\n"
                   "0\ta\t2\t5150\t7\n1\tb\t1\t1\t0\n2\tc\t1\t25\t11\n3\t*\t0\t%d\t12345\n" % (total - 5150 - 1 - 25))
    # against a per-base map, for the grid's regions
    regs = R.grid_regions()
    names, off, start, end, group = parse_regions(R.bed_text(regs, REFS, R.GRID_GROUPS), REFS, R.GRID_LENGTHS, True)
    n_regions, n_bases = R.merged_figures([(t, s, e, names.index(R.GRID_GROUPS[g])) for t, s, e, g in regs], R.GRID_LENGTHS, 4)
    rows = region_groups_text(names, start, end, group, R.GRID_LENGTHS, [0] * 4).splitlines()[1:]
    assert [r.split("\t")[2:4] for r in rows] == [[str(a), str(b)] for a, b in zip(n_regions, n_bases)]


def _parse_args(tmp_path, *extra):
    from mapdamage_amd.main import parse_args
    return parse_args(["-i", "x.bam", "-r", "x.fa", "-d", str(tmp_path / "out")] + list(extra))


@pytest.mark.parametrize("extra", [
    ("--regions", "a.bed", "--region-groups", "b.bed"),
    ("--regions", "a.bed", "--by-reference"),
    ("--regions", "a.bed", "--reference-groups", "g.tsv"),
    ("--region-groups", "a.bed", "--by-reference"),
    ("--region-groups", "a.bed", "--reference-groups", "g.tsv"),
    ("--regions", "a.bed", "--rescale-only"),
    ("--region-groups", "a.bed", "--rescale-only"),
    ("--only-regions",),
    ("--only-regions", "--by-reference"),
])
def test_argument_errors(tmp_path, capsys, extra):
    with pytest.raises(SystemExit) as err:
        _parse_args(tmp_path, *extra)
    assert err.value.code == 2
    assert "--regions" in capsys.readouterr().err


def test_arguments_and_the_options_become_regions(tmp_path):
    from mapdamage_amd.main import reference_strata
    from mapdamage_amd.tables import Regions
    o = _parse_args(tmp_path)
    assert o.regions is None and o.region_groups is None and o.only_regions is False
    assert reference_strata(o, REFS, LENS) is None
    bed = tmp_path / "p.bed"
    bed.write_text("chr2\t10\t20\tx\nchr1\t5\t9\ty\n")
    names, regions = reference_strata(_parse_args(tmp_path, "--region-groups", str(bed), "--only-regions"), REFS, LENS)
    assert names == ["x", "y", "*"] and isinstance(regions, Regions)
    assert regions.iv_off.tolist() == [0, 1, 2, 2, 2, 2] and regions.iv_group.tolist() == [1, 0] and regions.lengths == LENS
    names, regions = reference_strata(_parse_args(tmp_path, "--regions", str(bed)), REFS, LENS)
    assert names == ["regions", "*"] and regions.iv_group.tolist() == [0, 0]


def test_brute_force_helpers_on_hand_made_records():
    """The yardstick's own assignment (tests/regions_util.py), checked by hand on a few records."""
    from mapdamage_amd.batch import batch_from_records
    recs = [dict(flag=0, tid=0, pos=10, cigar=[(4, 5), (0, 10), (1, 3), (2, 2), (0, 5), (5, 4)], seq="A" * 23),   # [10, 27)
            dict(flag=0, tid=0, pos=50, cigar=[(4, 3)], seq="AAA"),                                               # [50, 51)
            dict(flag=0, tid=1, pos=0, cigar=[(7, 4), (3, 100), (8, 4)], seq="A" * 8),                            # [0, 108)
            dict(flag=4, tid=-1, pos=-1, cigar=[], seq="")]
    b = batch_from_records(recs)
    assert R.record_end(b).tolist() == [27, 51, 108, 0]
    regs = [(0, 27, 30, 0), (0, 26, 27, 1), (0, 50, 51, 0), (1, 107, 200, 1), (1, 5, 6, 0)]
    assert R.brute_group(b, regs, 2, 2).tolist() == [1, 0, 0, 2]
    assert R.brute_group(b, [(0, 27, 30, 0), (0, 51, 52, 0), (0, 0, 10, 0), (1, 108, 109, 0)], 2, 2).tolist() == [2, 2, 2, 2]
