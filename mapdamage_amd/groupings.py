"""The kinds of groups a run can have.  A run has one kind, and everything that depends on which one stands in that kind's
entry of ``KINDS``: the command line, the engine's set-up, the log and the writers ask the table, none branches on an option."""

from pathlib import Path
from typing import NamedTuple

import numpy as np

from .engine import DamageEngine


# what --by-terminal-damage and --by-pmd-score hand to ``DamageEngine.set_strata_damage`` and ``set_strata_pmd``
TerminalDamage = NamedTuple("TerminalDamage", [("positions", int), ("single_stranded", bool)])
PmdScore = NamedTuple("PmdScore", [("thresholds", tuple), ("model", tuple), ("single_stranded", bool)])


class Kind:
    """One kind of groups.  ``name``: ``DamageEngine.strata_kind``; ``options``: what selects it; ``companions``: the options
    that need it; ``label``: what the log calls its groups; ``directory``: where they are written, beside the usual three
    files.  ``payload(options, references, lengths)``: (group names, what ``apply(engine, payload, options)`` hands the
    engine); ``write(tables, options, strata, logger)``: the usual files and ``directory`` from a ``StratifiedTables``,
    returns the ``TableSet`` of the usual files."""
    companions = ()
    # --stats-only reads a folder and counts nothing.  It refuses --by-pmd-score and accepts and ignores the other grouping
    # options and their companions — an accident of the order parse_args once made its checks in, kept so that no command
    # line changes its fate.  This attribute is the whole of it.
    ignored_by_stats_only = True

    def given(self, options, which=None):
        """The options of this kind (``which``: of these) that the command line gives."""
        return [o for o in which or self.options if getattr(options, o[2:].replace("-", "_"), None) not in (None, False)]

    def prepare(self, options):
        """Checks and defaults of the kind's own options (``parse_args``); ValueError: the argument error."""

    def rank_words(self, engine):
        """uint64 words the ranks sum besides the tables and the kept reads (``take_rank_words``: their sum), or None."""


class ReferenceSequences(Kind):
    name, label, directory = "reference", "reference sequences", "by_reference"
    options = ("--by-reference", "--reference-groups")

    def payload(self, options, references, lengths):
        from .tables import groups_by_reference, parse_reference_groups
        if options.by_reference:
            return groups_by_reference(references)
        return parse_reference_groups(Path(options.reference_groups).read_text(), references)

    def apply(self, engine, payload, options):
        engine.set_strata(payload)

    def write(self, tables, options, strata, logger):
        tables.write(options.folder, strata[1], subdir=self.directory)
        return tables.merged


class RegionGroups(Kind):
    name, label, directory = "regions", "regions", "by_region"
    options, companions = ("--regions", "--region-groups"), ("--only-regions",)

    def payload(self, options, references, lengths):
        from . import tables
        names, *columns = tables.parse_regions(Path(options.regions or options.region_groups).read_text(), references, lengths,
                                               named=not options.regions)
        return names, tables.Regions(*columns, [int(x) for x in lengths])

    def apply(self, engine, payload, options):
        engine.set_strata_regions(payload.iv_off, payload.iv_start, payload.iv_end, payload.iv_group)

    def write(self, tables, options, strata, logger):
        from .tables import region_groups_text
        names, r = strata
        text = region_groups_text(names, r.iv_start, r.iv_end, r.iv_group, r.lengths, [tables.group_kept(g) for g in range(len(names))])
        # (--only-regions: the usual files from the named groups alone, summed on the host; by_region/ keeps '*')
        usual = tables.sum_of_groups(range(len(names) - 1)) if options.only_regions else None
        tables.write(options.folder, subdir=self.directory, groups_text=text, usual=usual)
        if getattr(options, "depth_regions_result", None) is not None:
            # (--depth-regions: the depth parted by the same intervals, beside groups.tsv)
            from . import depth
            depth.write_region_files(options.folder / self.directory, options.depth_result[0], names, r, options.depth_regions_result,
                                     options.depth_thresholds)
        return tables.merged if usual is None else usual


class TerminalDamageGroups(Kind):
    name, label, directory = "damage", "terminal damage", "by_damage"
    options, companions = ("--by-terminal-damage",), ("--terminal-positions",)

    def prepare(self, options):
        options.terminal_positions = 1 if options.terminal_positions is None else options.terminal_positions
        if options.terminal_positions > options.length:
            raise ValueError("--terminal-positions must not be greater than --length: the tables hold no position beyond it")

    def payload(self, options, references, lengths):
        return list(DamageEngine.DAMAGE_GROUPS), TerminalDamage(options.terminal_positions, bool(options.single_stranded))

    def apply(self, engine, payload, options):
        engine.set_strata_damage(payload.positions, payload.single_stranded)

    def write(self, tables, options, strata, logger):
        tables.write(options.folder, subdir=self.directory, groups_text=tables.kept_groups_text())
        (options.folder / self.directory / "conditional.tsv").write_text(tables.conditional_text(strata[1].single_stranded))
        return tables.merged


class PmdScoreGroups(Kind):
    name, label, directory = "pmd", "PMD score", "by_pmd"
    options, companions = ("--by-pmd-score",), ("--pmd-thresholds", "--pmd-model")
    ignored_by_stats_only = False

    def prepare(self, options):
        from . import pmd
        if options.minqual > 0:
            raise ValueError("--by-pmd-score cannot be combined with -Q / --min-basequal: the score weighs every base by its "
                             "quality, and under --min-basequal the decoders fold the mask into the bases and may drop the "
                             "quality column")
        try:
            options.pmd_thresholds = pmd.check_thresholds(
                [float(t) for t in ("3" if options.pmd_thresholds is None else options.pmd_thresholds).split(",")])
            model = [float(v) for v in ("0.3,0.01,0.001" if options.pmd_model is None else options.pmd_model).split(",")]
            if len(model) != 3:
                raise ValueError("--pmd-model takes three numbers: p,C,pi")
            options.pmd_model = pmd.check_model(*model)
        except ValueError as error:
            raise ValueError("--by-pmd-score: %s" % error) from None

    def payload(self, options, references, lengths):
        from .pmd import group_names
        return group_names(options.pmd_thresholds), PmdScore(tuple(options.pmd_thresholds), tuple(options.pmd_model),
                                                             bool(options.single_stranded))

    def apply(self, engine, payload, options):
        engine.set_strata_pmd(*payload, keep_scores=getattr(options, "tag_pmd_score", None) is not None)

    def write(self, tables, options, strata, logger):
        from .pmd import scores_text
        tables.write(options.folder, subdir=self.directory, groups_text=tables.kept_groups_text())
        (options.folder / self.directory / "scores.tsv").write_text(scores_text(tables.libraries, tables.pmd_hist))
        if tables.pmd_unqualified:
            logger.info("PMD scores: %d records without PHRED scores were scored with a base error of 0", tables.pmd_unqualified)
        return tables.merged

    def rank_words(self, engine):
        # (the score histogram and the records scored without qualities, summed as the kept reads are)
        return np.concatenate([engine.pmd_histogram().reshape(-1), np.array([engine.pmd_unqualified()], np.uint64)])

    def take_rank_words(self, tables, words):
        tables.pmd_hist, tables.pmd_unqualified = words[:-1].reshape(len(tables.libraries), -1), int(words[-1])


KINDS = (ReferenceSequences(), RegionGroups(), TerminalDamageGroups(), PmdScoreGroups())
OPTION_LIST = ", ".join(option for kind in KINDS for option in kind.options)


def kind_of(options):
    """The kind the options choose, or None."""
    return next((kind for kind in KINDS if kind.given(options)), None)


BY_NAME = {kind.name: kind for kind in KINDS}       # the kind an engine holds: BY_NAME[engine.strata_kind]
