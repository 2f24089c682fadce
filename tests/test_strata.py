"""Strata — tables per (library, group of reference sequences) — without a GPU: the groups file, the argument errors, the
by_reference/ layout and ``tables.StratifiedTables`` splitting and merging a block, against numpy sums."""

import numpy as np
import pytest

from mapdamage_amd import layout as L
from mapdamage_amd.tables import (StratifiedTables, TableSet, groups_by_reference, parse_reference_groups)

REFS = ["chr1", "chr2", "chrM", "scaf/1:a", "chr*"]


# ---------------------------------------------------------------------- the groups file
def test_groups_are_numbered_in_order_of_first_appearance_and_star_is_last():
    names, m = parse_reference_groups("chrM\tmito\nchr2\tnuclear\nchr1\tnuclear\n", REFS)
    assert names == ["mito", "nuclear", "*"]
    assert m.dtype == np.int32 and m.tolist() == [1, 1, 0, 2, 2]


def test_no_star_group_when_every_sequence_is_listed():
    text = "".join("%s\tg%d\n" % (r, i % 2) for i, r in enumerate(REFS))
    names, m = parse_reference_groups(text, REFS)
    assert names == ["g0", "g1"] and m.tolist() == [0, 1, 0, 1, 0]


def test_comments_empty_lines_and_odd_names():
    names, m = parse_reference_groups("# comment\n\nscaf/1:a\todd names\r\nchr*\todd names\n", REFS)
    assert names == ["odd names", "*"] and m.tolist() == [1, 1, 1, 0, 0]


def test_a_name_the_header_lacks_is_named():
    with pytest.raises(ValueError, match="chrX"):
        parse_reference_groups("chr1\ta\nchrX\tb\n", REFS)


def test_a_sequence_listed_twice_is_named():
    with pytest.raises(ValueError, match=r"line 3.*'chr1'.*twice"):
        parse_reference_groups("chr1\ta\nchr2\tb\nchr1\tb\n", REFS)


@pytest.mark.parametrize("line", ["chr1", "chr1\ta\tb", "chr1\t", "\ta", "chr1\t*"])
def test_malformed_lines(line):
    with pytest.raises(ValueError, match="line 1"):
        parse_reference_groups(line + "\n", REFS)


def test_by_reference_is_one_group_per_sequence():
    names, m = groups_by_reference(REFS)
    assert names == REFS and m.tolist() == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------------- the command line
def _parse(tmp_path, *extra):
    from mapdamage_amd.main import parse_args
    return parse_args(["-i", str(tmp_path / "x.bam"), "-r", str(tmp_path / "x.fa"), "-d", str(tmp_path / "out")] + list(extra))


def test_options_parse(tmp_path):
    assert _parse(tmp_path, "--by-reference").by_reference
    o = _parse(tmp_path, "--reference-groups", str(tmp_path / "g.tsv"))
    assert o.reference_groups == tmp_path / "g.tsv" and not o.by_reference
    o = _parse(tmp_path)
    assert not o.by_reference and o.reference_groups is None


@pytest.mark.parametrize("extra", [("--by-reference", "--rescale-only"), ("--reference-groups", "g.tsv", "--rescale-only"),
                                   ("--by-reference", "--reference-groups", "g.tsv")])
def test_argument_errors(tmp_path, extra, capsys):
    with pytest.raises(SystemExit) as err:
        _parse(tmp_path, *extra)
    assert err.value.code == 2
    assert "--by-reference" in capsys.readouterr().err


def test_help_says_these_are_no_reference_options(capsys):
    from mapdamage_amd.main import build_parser
    text = " ".join(build_parser().format_help().split())
    assert "--by-reference" in text and "--reference-groups" in text
    assert text.count("not a reference option") == 2


def test_reference_strata_from_options(tmp_path):
    from mapdamage_amd.main import reference_strata
    (tmp_path / "g.tsv").write_text("chr2\tb\n")
    names, m = reference_strata(_parse(tmp_path, "--reference-groups", str(tmp_path / "g.tsv")), REFS)
    assert names == ["b", "*"] and m.tolist() == [1, 0, 1, 1, 1]
    assert reference_strata(_parse(tmp_path), REFS) is None
    assert reference_strata(_parse(tmp_path, "--by-reference"), REFS)[0] == REFS


def test_too_many_tables_are_refused_with_a_message():
    from mapdamage_amd.engine import DamageEngine
    with pytest.raises(ValueError, match=r"70000 tables.*65535"):
        DamageEngine([("s", "l")], groups=["g%d" % i for i in range(70_000)])
    with pytest.raises(ValueError, match=r"70000 tables"):
        DamageEngine([("s", "l%d" % i) for i in range(7)], groups=["g%d" % i for i in range(10_000)])


# ---------------------------------------------------------------------- splitting and merging a block
LIBS = [("Zed", "libB"), ("Alpha", "libA")]
GROUPS = ["nuclear", "mito", "*"]
LEN, AROUND, LGD = 6, 3, 40


def _block(seed=5):
    rng = np.random.default_rng(seed)
    n = len(LIBS) * len(GROUPS)
    mis = rng.integers(0, 1000, (n, 2, 2, LEN, L.N_MIS_COLS)).astype(np.uint64)
    comp = rng.integers(0, 1000, (n, 2, 2, LEN + AROUND, 4)).astype(np.uint64)
    lgd = rng.integers(0, 3, (n, 2, 2, LGD)).astype(np.uint64)
    # out-of-range lengths: (stratum, kind, strand, length)
    over = np.asarray([[0, 1, 0, 70000], [4, 0, 1, 80000], [5, 1, 1, 90000], [4, 0, 1, 80000]], np.int64)
    strata = TableSet([lib for lib in LIBS for _ in GROUPS], LEN, AROUND, mis, comp, lgd, over, 12345)
    kept = np.arange(10, 10 + n, dtype=np.uint64)
    return strata, kept


def test_split_and_merge_against_numpy_sums():
    strata, kept = _block()
    st = StratifiedTables.from_block(strata, LIBS, GROUPS, kept)
    ng = len(GROUPS)
    for g, name in enumerate(GROUPS):
        t = st.group(g)
        assert t.libraries == LIBS
        for li in range(len(LIBS)):
            np.testing.assert_array_equal(t.mis[li], strata.mis[li * ng + g])
            np.testing.assert_array_equal(t.comp[li], strata.comp[li * ng + g])
            np.testing.assert_array_equal(t.lgd[li], strata.lgd[li * ng + g])
        assert t.n_kept == int(kept[g]) + int(kept[ng + g])
        np.testing.assert_array_equal(st.group(name).mis, t.mis)
    assert st.group(0).lgd_over.tolist() == [[0, 1, 0, 70000]]
    assert st.group(1).lgd_over.tolist() == [[1, 0, 1, 80000], [1, 0, 1, 80000]]
    assert st.group(2).lgd_over.tolist() == [[1, 1, 1, 90000]]
    m = st.merged
    assert m.libraries == LIBS and m.n_kept == 12345 and st.n_kept == 12345
    for li in range(len(LIBS)):
        np.testing.assert_array_equal(m.mis[li], strata.mis[li * ng:(li + 1) * ng].sum(axis=0))
        np.testing.assert_array_equal(m.comp[li], strata.comp[li * ng:(li + 1) * ng].sum(axis=0))
        np.testing.assert_array_equal(m.lgd[li], strata.lgd[li * ng:(li + 1) * ng].sum(axis=0))
    assert m.mis.dtype == np.uint64
    assert sorted(m.lgd_over.tolist()) == [[0, 1, 0, 70000], [1, 0, 1, 80000], [1, 0, 1, 80000], [1, 1, 1, 90000]]
    # the merged block is the sum of the groups, the emitted text too (the lengths beyond the dense histogram included)
    total = st.group(0)
    for g in (1, 2):
        total.add(st.group(g))
    np.testing.assert_array_equal(total.mis, m.mis)
    assert total.lgdistribution_text() == m.lgdistribution_text()


def test_groups_tsv_and_the_directory_layout(tmp_path):
    strata, kept = _block()
    st = StratifiedTables.from_block(strata, LIBS, GROUPS, kept)
    group_of_tid = [0, 0, 1, 2, 2, 0]
    st.write(tmp_path, group_of_tid)
    assert (tmp_path / "by_reference" / "groups.tsv").read_text() == (
        "Index\tGroup\tSequences\tReads\n0\tnuclear\t3\t%d\n1\tmito\t1\t%d\n2\t*\t2\t%d\n" % (10 + 13, 11 + 14, 12 + 15))
    assert sorted(p.name for p in (tmp_path / "by_reference").iterdir()) == ["0", "1", "2", "groups.tsv"]
    for g in range(3):
        t = st.group(g)
        d = tmp_path / "by_reference" / str(g)
        assert sorted(p.name for p in d.iterdir()) == ["dnacomp.txt", "lgdistribution.txt", "misincorporation.txt"]
        assert (d / "misincorporation.txt").read_text() == t.misincorporation_text()
        assert (d / "dnacomp.txt").read_text() == t.dnacomp_text()
        assert (d / "lgdistribution.txt").read_text() == t.lgdistribution_text()
    assert (tmp_path / "misincorporation.txt").read_text() == st.merged.misincorporation_text()
    assert (tmp_path / "dnacomp.txt").read_text() == st.merged.dnacomp_text()
    assert (tmp_path / "lgdistribution.txt").read_text() == st.merged.lgdistribution_text()


def test_a_block_of_the_wrong_size_is_refused():
    strata, _ = _block()
    with pytest.raises(AssertionError):
        StratifiedTables.from_block(strata, LIBS, GROUPS[:2])
