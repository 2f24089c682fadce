"""The table of the kinds of groups (mapdamage_amd/groupings.py) as the command line sees it: a run has one kind, the kinds
belong to the tabulation pass, ``--write-groups`` / ``--tag-group`` want any one of them, and every directory a kind writes is
one the Bayesian estimate visits."""

import itertools

import pytest

from mapdamage_amd import groupings

# every grouping option with the argument it takes
OPTIONS = {"--by-reference": (), "--reference-groups": ("g.tsv",), "--regions": ("a.bed",), "--region-groups": ("b.bed",),
           "--by-terminal-damage": (), "--by-pmd-score": ()}


def _argv(tmp_path, *extra):
    return ["-i", str(tmp_path / "x.bam"), "-r", str(tmp_path / "x.fa"), "-d", str(tmp_path / "out")] + [str(x) for x in extra]


def _refused(tmp_path, capsys, *extra):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as err:
        parse_args(_argv(tmp_path, *extra))
    assert err.value.code == 2
    return capsys.readouterr().err


def test_the_table_lists_the_six_options():
    assert sorted(option for kind in groupings.KINDS for option in kind.options) == sorted(OPTIONS)
    assert groupings.OPTION_LIST.split(", ") == [option for kind in groupings.KINDS for option in kind.options]


@pytest.mark.parametrize("first,second", list(itertools.permutations(OPTIONS, 2)))
def test_two_grouping_options_exclude_each_other(tmp_path, capsys, first, second):
    message = _refused(tmp_path, capsys, first, *OPTIONS[first], second, *OPTIONS[second])
    assert "exclude each other" in message
    # (the options as words of the message: "--regions" is no part of "--region-groups")
    words = message.replace(",", " ").split()
    assert first in words and second in words


@pytest.mark.parametrize("option", list(OPTIONS))
def test_a_grouping_option_belongs_to_the_tabulation_pass(tmp_path, capsys, option):
    message = _refused(tmp_path, capsys, option, *OPTIONS[option], "--rescale-only")
    assert option in message and "--rescale-only" in message


@pytest.mark.parametrize("option", list(OPTIONS))
def test_write_groups_and_tag_group_take_any_kind(tmp_path, option):
    from mapdamage_amd.main import parse_args
    out = tmp_path / "kept.bam"
    o = parse_args(_argv(tmp_path, option, *OPTIONS[option], "--write-kept", out, "--write-groups", "1,0", "--tag-group", "XG"))
    assert o.write_groups == (0, 1) and o.tag_group == "XG"
    assert groupings.kind_of(o) is not None and option in groupings.kind_of(o).options


def test_write_groups_and_tag_group_need_a_kind(tmp_path, capsys):
    out = tmp_path / "kept.bam"
    for extra in (("--write-groups", "0"), ("--tag-group", "XG")):
        message = _refused(tmp_path, capsys, "--write-kept", out, *extra)
        assert extra[0] + " needs a run with groups" in message
        assert all(option in message for option in OPTIONS)


def test_stats_only_ignores_every_kind_but_the_pmd_score(tmp_path, capsys):
    from mapdamage_amd.main import parse_args
    (tmp_path / "out").mkdir()
    (tmp_path / "out" / "dnacomp_genome.csv").write_text("")
    for option, args in OPTIONS.items():
        if option == "--by-pmd-score":
            assert "--stats-only" in _refused(tmp_path, capsys, option, "--stats-only", "--fix-nicks")
        else:
            assert parse_args(_argv(tmp_path, option, *args, "--stats-only", "--fix-nicks")).stats_only


def test_the_estimate_visits_every_directory_the_table_declares(tmp_path, monkeypatch):
    """A folder with one group directory per kind: ``bayesian_estimates`` hands all of them to the estimator."""
    import logging
    from types import SimpleNamespace
    from mapdamage_amd import main, stats
    directories = [kind.directory for kind in groupings.KINDS]
    assert len(set(directories)) == len(groupings.KINDS) == 4 and all(directories)
    folder = tmp_path / "out"
    for sub in directories:
        (folder / sub / "0").mkdir(parents=True)
        (folder / sub / "groups.tsv").write_text("Index\tGroup\tReads\n0\tg\t1\n")
        (folder / sub / "0" / "misincorporation.txt").write_text("")
    seen = []
    monkeypatch.setattr(main, "_base_frequencies", lambda *a, **k: None)
    monkeypatch.setattr(main, "_group_has_data", lambda group: True)
    monkeypatch.setattr(stats, "estimate_folders", lambda folders, *a, **k: seen.extend(folders))
    options = SimpleNamespace(folder=folder, stats_chain=0, stats_options=None)
    assert main.bayesian_estimates(options, logging.getLogger("test_groupings")) == 0
    assert seen == [folder] + [folder / sub / "0" for sub in directories]
