"""Mirror of the reference's command line for the tabulation pass (mapdamage/main.py:49-266,
mapdamage/config.py:80-494): same flags, same defaults, same output files
(``misincorporation.txt``, ``dnacomp.txt``, ``lgdistribution.txt``, ``Runtime_log.txt``), with the
per-read loop replaced by ``DamageEngine`` (HIP).  R plotting, the Bayesian stage and rescaling
are out of scope: their flags are parsed, and asking for them is an error."""

import argparse
import dataclasses
import logging
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

from . import __version__, groupings
from . import depth as depth_files
from . import pileup as pileup_files
from .batch import mark_unmaskable
from .engine import BadReadError, DamageEngine, MdxError
from .groupings import PmdScore, TerminalDamage        # noqa: F401  (where callers import them from)
from .fasta import compare_sequence_dicts, ensure_fasta_index, is_bgzf, is_plain_gzip, read_fasta_index, reference_for_bam
from .layout import FLAG_FILTER
from .reader import BAMReader, draw_uniform, is_stream
from .sam import MASK_WHAT, SAM_BGZF, SAM_GZIP, BAMError, KeptIndexError, KeptTagClash
from .statistics import check_table_and_warn_if_dmg_freq_is_low

_LOG_FORMAT = "%(asctime)s %(name)s %(levelname)s %(message)s"


class _Stages:
    """MDX_STAGE_LOG=<file>: the wall-clock time (``time.time()``) at which each stage of the run was reached, as one JSON
    object — what bench.py's ``cli_wall`` splits a cold run of this command into.  Costs a dictionary entry per stage."""

    def __init__(self):
        import os
        self.path = os.environ.get("MDX_STAGE_LOG")
        self.marks = []

    def mark(self, label):
        if self.path:
            self.marks.append((label, time.time()))

    def write(self):
        if self.path:
            import json
            with open(self.path, "w") as fh:
                json.dump({"stages": self.marks}, fh)


def _warm_up(device, pinned_bytes):
    """On a helper thread beside the header and index reads: the device's context, the decode kernels' code object, the
    inflating threads and the pinned buffer of the host's share (include/mdx.h ``mdx_warm``; ctypes drops the GIL)."""
    from .engine import load_library
    try:
        load_library().mdx_warm(device, pinned_bytes)
    except Exception:       # (a run that cannot warm up finds out why when it creates its engine)
        pass


def _ranged(cls, lo=float("-inf"), hi=float("inf")):
    def parse(value):
        value = cls(value)
        if value < lo:
            raise argparse.ArgumentTypeError("must be greater than or equal to %s" % (lo,))
        if value > hi:
            raise argparse.ArgumentTypeError("must be less than or equal to %s" % (hi,))
        return value
    return parse


def _flag_mask(value):
    """A flag mask of the command line: decimal or 0x hex, 0..65535."""
    try:
        mask = int(value, 16) if value.lower().startswith("0x") else int(value, 10)
    except ValueError:
        raise argparse.ArgumentTypeError("must be a decimal or 0x hexadecimal number")
    if not 0 <= mask <= 65535:
        raise argparse.ArgumentTypeError("must lie in 0..65535")
    return mask


def build_parser():
    p = argparse.ArgumentParser(prog="mapDamage", usage="%(prog)s [options] -i alignment.bam -r reference.fasta")
    p.add_argument("--version", action="version", version="%(prog)s (mapdamage_amd " + __version__ + ")")
    g = p.add_argument_group("Input and output")
    g.add_argument("-i", "--input", dest="filename", type=Path, metavar="SAM/BAM")
    g.add_argument("-r", "--reference", dest="ref", type=Path, metavar="FASTA")
    g.add_argument("-d", "--folder", type=Path)
    g.add_argument("-n", "--downsample", type=float, metavar="X")
    g.add_argument("--downsample-seed", type=int, metavar="X")
    g = p.add_argument_group("General options")
    g.add_argument("--merge-libraries", action="store_true")
    g.add_argument("--merge-reference-sequences", action="store_true", help=argparse.SUPPRESS)
    g.add_argument("-l", "--length", type=_ranged(int, 1), default=70)
    g.add_argument("-a", "--around", type=_ranged(int, 0), default=10)
    g.add_argument("-Q", "--min-basequal", dest="minqual", type=_ranged(int, 0, 93), default=0)
    g.add_argument("--plot-only", action="store_true")
    g.add_argument("--log-level", default="INFO", type=str.upper, choices=("DEBUG", "INFO", "WARNING", "ERROR"))
    g.add_argument("--no-plot", dest="no_r", action="store_true", help=argparse.SUPPRESS)
    g = p.add_argument_group("Options for graphics")
    g.add_argument("-y", "--ymax", type=float, default=0.3)
    g.add_argument("-m", "--readplot", type=_ranged(int, 1), default=25)
    g.add_argument("-b", "--refplot", type=_ranged(int, 1), default=10)
    g.add_argument("-t", "--title")
    g = p.add_argument_group("Options for the statistical estimation")
    for flag, typ, default in (("--rand", int, 30), ("--burn", int, 10000), ("--adjust", int, 10),
                               ("--iter", int, 50000), ("--seq-length", int, 12)):
        g.add_argument(flag, type=typ, default=default)
    g.add_argument("--termini", choices=("5p", "3p", "both"), default="both")
    g.add_argument("--stats", action="store_true",
                   help="estimate the damage parameters once the tables are written (mapdamage/r/stats/ on the GPU, one chain per "
                        "table set in one launch): Stats_out_MCMC_iter.csv, ..._iter_summ_stat.csv and ..._correct_prob.csv; needs "
                        "one of --fix-nicks, --use-raw-nick-freq and --single-stranded.  With --by-reference / --reference-groups / "
                        "--regions / --region-groups / --by-terminal-damage every group gets a chain of its own and its three files "
                        "beside its tables")
    g.add_argument("--stats-seed", type=int, default=0, metavar="N",
                   help="seed of the estimate's random numbers (Philox4x32-10; a chain is reproducible from it)")
    g.add_argument("--stats-chain", type=int, default=0, help=argparse.SUPPRESS)     # key word of the run's own chain (group g: g + 1)
    for flag in ("--forward", "--reverse", "--var-disp", "--jukes-cantor", "--diff-hangs", "--fix-nicks",
                 "--use-raw-nick-freq", "--single-stranded", "--theme-bw", "--stats-only", "--no-stats",
                 "--check-R-packages"):
        g.add_argument(flag, action="store_true")
    g = p.add_argument_group("Options for rescaling of BAM files")
    g.add_argument("--rescale", action="store_true")
    g.add_argument("--rescale-only", action="store_true")
    g.add_argument("--rescale-out", type=Path)
    g.add_argument("--rescale-length-5p", type=int)
    g.add_argument("--rescale-length-3p", type=int)
    g = p.add_argument_group("MI355X engine")
    g.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    g.add_argument("--gpus", type=_ranged(int, 1), default=1,
                   help="tabulate on this many GPUs of the node: one process per GPU (the command re-executes itself under "
                        "torch.distributed.run unless it was launched that way), the records sharded by slab of the file, the "
                        "tables summed with one RCCL all-reduce, rank 0 writes the output files")
    g.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                   help="torch.distributed backend of the table reduction: nccl = RCCL over xGMI; gloo sums on the host")
    g.add_argument("--share-gpu", action="store_true",
                   help="every rank uses --device instead of its own GPU (tests of the multi-rank path on a 1-GPU box; "
                        "needs --dist-backend gloo: RCCL refuses two ranks on one device)")
    g.add_argument("--print-launch", action="store_true",
                   help="with --gpus N > 1: print the torchrun command the run would re-execute itself under, and exit")
    g.add_argument("--freq-files", action="store_true",
                   help="EXPERIMENTAL: also write 5pCtoT_freq.txt / 3pGtoA_freq.txt (mapDamage 2.0-2.2 outputs that "
                        "this reference snapshot no longer produces; format unpinned)")
    g.add_argument("--by-reference", action="store_true",
                   help="also tabulate every reference sequence of the header on its own, in the same pass: the usual three files "
                        "are what the run writes without the option, and by_reference/ holds groups.tsv and the three files of each "
                        "sequence in a directory named by its index (not a reference option: mapdamage/config.py has none; "
                        "mapDamage 2.0 printed a Chr column for this)")
    g.add_argument("--reference-groups", type=Path, metavar="TSV",
                   help="like --by-reference for groups of sequences: lines 'sequence name<TAB>group name'; the sequences not "
                        "listed form a last group named '*' (not a reference option either)")
    g.add_argument("--regions", type=Path, metavar="BED",
                   help="also tabulate the records that overlap the regions of a BED file (sequence<TAB>start<TAB>end, 0-based, "
                        "half-open) apart from the rest, in the same pass: a record occupies [pos, pos + max(1, reference bases of "
                        "its CIGAR)) and belongs to the first region it shares a base with, as `samtools view -L` decides; the usual "
                        "three files are what the run writes without the option, and by_region/ holds groups.tsv and the three files "
                        "of the groups 'regions' and '*' (everything else) in directories named by their index")
    g.add_argument("--region-groups", type=Path, metavar="BED",
                   help="like --regions with the group of a region named by column 4 of the BED file; overlapping regions of "
                        "different groups are an error, a record that overlaps several goes to the one that begins first")
    g.add_argument("--only-regions", action="store_true",
                   help="with --regions / --region-groups: the usual three files hold the records inside the regions only (the sum "
                        "of the named groups, '*' left out) — what `samtools view -L BED` in front would have produced; by_region/ "
                        "is still complete")
    g.add_argument("--by-terminal-damage", action="store_true",
                   help="also tabulate the records apart by the damage their own ends show, in the same pass: a record is "
                        "5p-damaged if it adds to C>T within the first --terminal-positions positions of the 5p table, 3p-damaged "
                        "if it adds to G>A within those of the 3p table (C>T with --single-stranded), by every rule the tables "
                        "follow (clips, gaps, strand, --min-basequal); the usual three files are what the run writes without the "
                        "option, and by_damage/ holds groups.tsv, the three files of the groups none, 5p, 3p and both in "
                        "directories named by their index, and conditional.tsv: the substitution frequency at one end given the "
                        "other end's state, which tells a damaged library from a contaminated one.  Not a reference option: "
                        "mapdamage/config.py has none")
    g.add_argument("--terminal-positions", type=_ranged(int, 1), default=None, metavar="K",
                   help="with --by-terminal-damage: the positions from either end that decide a record's group (default 1, at "
                        "most --length).  Not a reference option either")
    g.add_argument("--by-pmd-score", action="store_true",
                   help="also tabulate the records apart by their post-mortem damage score (PMDS; Skoglund et al. 2014, PNAS "
                        "111:2229), in the same pass: the log-likelihood ratio, over the record's whole alignment and with its "
                        "base qualities, that it carries deamination damage — C>T from its 5p end, G>A from its 3p end (C>T "
                        "with --single-stranded).  The usual three files are what the run writes without the option; by_pmd/ "
                        "holds groups.tsv, the three files of the records below, between and at or above the --pmd-thresholds in "
                        "directories named by their index, and scores.tsv: the score distribution per library in half-unit bins. "
                        "What `pmdtools --threshold T` in front of the run would have kept is the last group.  Not with "
                        "--min-basequal, whose mask replaces the qualities the score reads.  Not a reference option: "
                        "mapdamage/config.py has none")
    g.add_argument("--pmd-thresholds", default=None, metavar="T[,T...]",
                   help="with --by-pmd-score: 1 to 15 strictly increasing scores that part the groups (default 3; a list that begins with a "
                        "negative number is written --pmd-thresholds=-1,3)")
    g.add_argument("--pmd-model", default=None, metavar="p,C,pi",
                   help="with --by-pmd-score: the damage model D_z = p (1-p)^(z-1) + C at distance z from the end and the "
                        "polymorphism rate pi (default 0.3,0.01,0.001; 0 < p < 1, 0 <= C, p + C < 1, 0 < pi < 1)")
    g.add_argument("--min-mapq", type=_ranged(int, 0, 255), default=0, metavar="Q",
                   help="drop the records whose MAPQ is below Q, as `samtools view -q Q` in front would (numeric: 255 passes any Q); "
                        "evaluated by the decoders, on the device where the file is decoded there.  Not a reference option "
                        "(mapdamage/config.py has none), like the four below.  The filters apply to every record in front of "
                        "everything else — the flag filter 0xF04 of the reference still applies on top, --downsample draws once per "
                        "record that is left; Runtime_log.txt and record_filters.tsv give the records dropped by each.  --rescale "
                        "tabulates and estimates from the filtered records and still rewrites every record of the input")
    g.add_argument("--require-flags", type=_flag_mask, default=0, metavar="F",
                   help="drop the records that lack one of the bits of F (decimal or 0x hex, 0..65535; `samtools view -f F`), on the 16 "
                        "bits the file carries")
    g.add_argument("--exclude-flags", type=_flag_mask, default=0, metavar="F",
                   help="drop the records that have one of the bits of F (`samtools view -F F`)")
    g.add_argument("--min-read-length", type=_ranged(int, 0, 2**31 - 1), default=0, metavar="L",
                   help="drop the records whose SEQ field is shorter than L bases (BAM's l_seq; a SAM '*' is 0) — the length of the "
                        "stored sequence, not the query length of the CIGAR")
    g.add_argument("--max-read-length", type=_ranged(int, 0, 2**31 - 1), default=0, metavar="L",
                   help="drop the records whose SEQ field is longer than L bases (0: no upper bound)")
    g.add_argument("--write-kept", type=Path, default=None, metavar="BAM",
                   help="also write the records the run counts to a BAM file, in the same pass: those the flag filter 0xF04, the "
                        "record filters and --downsample to a fraction leave, in the input's order, every record byte for byte as "
                        "the input has it, under the input's header (no @PG line is added).  Selected, compacted and compressed on "
                        "the device, so BAM input on the device decode path only: not SAM text, --host-decode, --gpus above 1 or "
                        "-n N.  The tables and logs are what the run writes without the option; write_kept.tsv gives the records "
                        "and bytes written.  Not a reference option: mapdamage/config.py has none")
    g.add_argument("--write-groups", default=None, metavar="I[,I...]",
                   help="with --write-kept in a run that has groups (" + groupings.OPTION_LIST + "): write only the records of the groups with these indices of "
                        "groups.tsv, for all libraries — `--by-pmd-score --pmd-thresholds 3 --write-groups 1` is what `pmdtools "
                        "--threshold 3` would have written (default: every counted record)")
    g.add_argument("--tag-group", default=None, metavar="TAG",
                   help="with --write-kept in a run that has groups: append TAG:S (uint16) to every written record, its group's "
                        "index in groups.tsv — the number --write-groups takes —, so that one file of one pass carries the "
                        "partition (`samtools view -d TAG:1` splits it afterwards).  TAG: two characters, [A-Za-z][A-Za-z0-9]; a "
                        "written record that has such a tag already ends the run")
    g.add_argument("--tag-pmd-score", default=None, metavar="TAG",
                   help="with --write-kept --by-pmd-score: append TAG:f to every written record, its PMD score (the run's "
                        "fixed-point score as the nearest float32), so that the file can be split at any threshold afterwards")
    g.add_argument("--write-index", action="store_true",
                   help="with --write-kept: also write the BAI index of that file, BAM.bai, from the offsets and coordinates the "
                        "run has on the device — what `samtools index BAM` behind the run would make by inflating the file "
                        "again.  The written records must be in coordinate order and lie inside the first 2^29 bases of their "
                        "reference sequences (BAI's limit; CSI is not written); the first one that does not ends the run")
    g.add_argument("--mask-ends", default=None, metavar="K5[,K3]",
                   help="with --write-kept: hand the written records on with the damaged ends of their molecules masked — base N, "
                        "quality 0 — inside the first K5 query bases of the molecule's 5' end and the last K3 of its 3' end (one "
                        "number: both; 0..255 each, not both 0).  A reverse-strand record's 5' end is its stored right end.  The "
                        "windows count query bases (SEQ without its soft clips), not the tables' positions: gap columns are not "
                        "counted.  No record changes its length and no tag (NM, MD) is touched, as `bam trimBam` leaves them; the "
                        "tables, groups and tags are those of the reads as they are.  mask_ends.tsv gives the records and bases "
                        "masked.  Not a reference option")
    g.add_argument("--mask-what", choices=MASK_WHAT, default=None,
                   help="with --mask-ends: `all` bases of the windows (the default); the `transitions` alone, T in the 5' window and "
                        "A in the 3' window of the molecule's own strand (T in both with --single-stranded); or those of them that "
                        "are `mismatches`, with C or G in the reference underneath — which keeps the true T and A, and with them the "
                        "bias towards the reference that `transitions` does not have")
    g.add_argument("--calmd", action="store_true", default=False,
                   help="with --write-kept: every written record leaves with NM and MD recomputed against the run's reference, as "
                        "`samtools calmd` behind the run would — from the bytes the file will hold, so behind --mask-ends and with "
                        "the tags of --tag-group / --tag-pmd-score in place.  Every NM and MD field a record had is removed, and "
                        "NM (the smallest unsigned type) and MD:Z follow its other tags; a record the rule cannot follow (a CIGAR "
                        "that does not fill SEQ, a place outside the reference, tags that cannot be walked, CG:B) is written as it "
                        "is.  An ambiguity code of the reference appears in MD as N.  calmd.tsv gives the records recomputed and "
                        "skipped.  Not a reference option")
    g.add_argument("--remove-duplicates", action="store_true", default=False,
                   help="drop the later copies of a molecule before anything is counted, in the same pass: among the unpaired "
                        "records the flag filter, the record filters and --downsample to a fraction leave, those of one library "
                        "that share sequence, strand and both unclipped ends (the leading and trailing S and H operations counted "
                        "in, as DeDup, `rmdup_collapsed` and `samtools markdup` take the ends) are one molecule; the first in the "
                        "input's order is counted, every later one gets flag 0x400 on the device, which the flag filter 0xF04 "
                        "drops from the tables, every kind of groups and the file of --write-kept.  Exact — the fields are "
                        "compared, not a hash of them — and the same whatever the slabs.  Paired records are not examined.  "
                        "duplicates.tsv and duplicates_histogram.tsv give the counts per library.  BAM input on the device decode "
                        "path only: not SAM text, --host-decode, --gpus above 1 or -n N; at most 2^30 records in the input.  Not "
                        "a reference option")
    g.add_argument("--duplicate-ends", choices=DUPLICATE_ENDS, default=None,
                   help="with --remove-duplicates: `both` ends of the molecule (the default: merged reads, whose two ends are the "
                        "molecule's), or the `5p` end alone — the unclipped start of a forward record, the unclipped end of a "
                        "reverse one —, as `samtools rmdup -s` does for single-end reads whose 3' end is where sequencing stopped")
    g.add_argument("--depth", action="store_true", default=False,
                   help="depth of coverage of the counted records, in the same pass: every record the flag filter, the record "
                        "filters, --downsample to a fraction and --remove-duplicates leave, whose library is known and whose "
                        "alignment lies inside its sequence, covers the reference bases of its M, = and X operations (D and N "
                        "advance without covering, as `samtools depth` without -J).  coverage.tsv gives per sequence and for "
                        "the whole reference the reads, covered bases, breadth, aligned bases, mean and largest depth; "
                        "depth_histogram.tsv the reference bases at every depth.  Takes 4 bytes of device memory per reference "
                        "base.  The groups of a run do not part it.  BAM input on the device decode path only: not SAM text, "
                        "--host-decode, --gpus above 1 or -n N.  Not a reference option")
    g.add_argument("--depth-bedgraph", metavar="PATH", default=None,
                   help="with --depth: the stretches of equal depth above 0 as `name start end depth` lines, what `bedtools "
                        "genomecov -bg` writes; written under a temporary name and moved into place at the end")
    g.add_argument("--depth-regions", action="store_true", default=False,
                   help="with --depth and --regions / --region-groups: the depth on target, from the same pass.  Every reference "
                        "base belongs to the region that holds it (after the merging of a group's overlapping and abutting "
                        "regions) and to that region's group, or to '*' — base by base, so a read that hangs over a region's edge "
                        "adds its outside bases to '*', whichever group its record is counted in.  by_region/ gets coverage.tsv "
                        "(per group: bases, covered, breadth, aligned bases, mean and largest depth), depth_histogram.tsv and "
                        "depth_thresholds.tsv (per group) and regions_depth.tsv (a line per region: what `samtools bedcov` or "
                        "`mosdepth --by` give)")
    g.add_argument("--depth-thresholds", metavar="T[,T...]", default=None,
                   help="with --depth-regions: the depths T for which depth_thresholds.tsv gives the bases at depth >= T; strictly "
                        "increasing integers in 1..1022, at most 32 (default: 1,5,10,20)")
    g.add_argument("--pileup-sites", metavar="FILE", default=None,
                   help="allele counts and a pseudo-haploid call at the sites of FILE, in the same pass: what `samtools mpileup -l "
                        "FILE | pileupCaller` makes of the counted records, without writing them first.  Lines of "
                        "sequence<TAB>position[<TAB>ref<TAB>alt[<TAB>id]], the position 1-based, in any order; `#` lines and empty "
                        "lines are skipped.  A record is counted as for --depth; at every site it lies over, its base goes to one "
                        "of A+ C+ G+ T+ A- C- G- T- (as stored; the strand by FLAG 0x10), Deletions, LowQual, Other or Masked.  "
                        "pileup.tsv gives a line per site in (sequence, position) order, pileup_summary.tsv the totals.  Takes 48 "
                        "bytes of device memory per site.  Libraries and groups are summed.  BAM input on the device decode path "
                        "only: not SAM text, --host-decode, --gpus above 1 or -n N.  Not a reference option")
    g.add_argument("--pileup-min-basequal", metavar="Q", type=int, default=None,
                   help="with --pileup-sites: a base whose quality is below Q counts as LowQual (0..93, default 0); a record "
                        "without qualities is never LowQual.  With --min-basequal as well, Q must not be above it")
    g.add_argument("--pileup-mask-ends", metavar="K5[,K3]", default=None,
                   help="with --pileup-sites: a base inside the first K5 query bases of the molecule's 5' end or the last K3 of its "
                        "3' end counts as Masked (0..255 each, one number means both, default 0,0): the windows of --mask-ends "
                        "with --mask-what all")
    g.add_argument("--pileup-call", choices=pileup_files.CALLS, default=None,
                   help="with --pileup-sites: `random` (the default) draws one of the site's eligible bases, `majority` takes the "
                        "most frequent one and draws among ties, `none` leaves the Call column out.  The draw is a function of "
                        "the site's counters, --pileup-seed, the sequence and the position alone")
    g.add_argument("--pileup-seed", metavar="N", type=int, default=None, help="with --pileup-sites: the seed of the draws (default 0)")
    g.add_argument("--pileup-min-depth", metavar="D", type=int, default=None,
                   help="with --pileup-sites: a site with fewer than D eligible bases is called N (default 1)")
    g.add_argument("--pileup-likelihoods", action="store_true", default=False,
                   help="with --pileup-sites: the ten diploid genotype likelihoods at every site, from the same pass: what `angsd "
                        "-GL 2 -doGlf 2 -sites FILE` makes of the counted records (GATK's model).  A base adds where it adds to a "
                        "base counter of pileup.tsv, so --pileup-min-basequal and --pileup-mask-ends shape them too; "
                        "--pileup-single-strand-mode chooses the strands.  pileup_likelihoods.tsv gives log10 ratios to the best "
                        "genotype, pileup_likelihoods_summary.tsv the totals.  Takes 192 bytes of HBM per site more.  Not beside -Q")
    g.add_argument("--pileup-noqual-quality", metavar="Q", type=int, default=None,
                   help="with --pileup-likelihoods: the quality of the bases of a record without qualities (1..93, default 30)")
    g.add_argument("--pileup-beagle", metavar="PATH", default=None,
                   help="with --pileup-likelihoods and sites that bring ref and alt: the BEAGLE genotype likelihood file of `angsd "
                        "-doGlf 2` — ref/ref, ref/alt, alt/alt per site, normalised — for PCAngsd, NGSadmix, ngsRelate; gzip if "
                        "PATH ends in .gz")
    g.add_argument("--pileup-damage-profile", metavar="FILE", default=None,
                   help="with --pileup-likelihoods: a misincorporation.txt, this program's or mapDamage's, usually that of a first run "
                        "over the same file: its C>T rates by distance from the 5' end and G>A rates by distance from the 3' end enter "
                        "the error model (as in ATLAS and snpAD), so a T over a C near a read's start counts as the deamination it "
                        "probably is, and no base has to be masked.  Distances count query bases, as --pileup-mask-ends does.  "
                        "pileup_damage_profile.tsv lists the rates used.  Takes 160 instead of 192 bytes of HBM per site.  Not beside "
                        "--single-stranded")
    g.add_argument("--pileup-damage-positions", metavar="K", type=int, default=None,
                   help="with --pileup-damage-profile: the positions from either end that keep their own rate; every base further in "
                        "takes the pooled rate of the positions K+1 and up (1..254 and below the table's --length; default 20)")
    g.add_argument("--pileup-single-strand-mode", action="store_true", default=False,
                   help="with --pileup-sites whose lines bring ref and alt: at a C/T site only the bases of reverse-strand records "
                        "are eligible, at a G/A site only those of forward-strand records (pileupCaller --singleStrandMode)")
    g.add_argument("--batch-reads", type=int, default=4_000_000, help="records per device batch")
    g.add_argument("--gpu-decode", dest="gpu_decode", action="store_true", default=True,
                   help="inflate and unpack a BAM file on the GPU (include/mdx.h mdx_gbam_*): the compressed file goes "
                        "to HBM, the batch columns never exist on the host (the default; SAM input and --downsample to a fixed "
                        "number of reads are decoded on the host)")
    g.add_argument("--host-decode", dest="gpu_decode", action="store_false",
                   help="decode on the host (multi-threaded BGZF/BAM decoder) even where the GPU path applies")
    g.add_argument("--host-deflate", action="store_true",
                   help="--rescale-only: deflate the output's BGZF blocks with zlib (level 6) on the host's threads, as htslib does "
                        "behind the reference, instead of on the device (the default: four times as fast, the file 3 %% larger; the "
                        "records are the same)")
    g.add_argument("--chunk-mb", type=_ranged(float, 0), default=1024,
                   help="decode a BAM file in chunks of this many MiB of uncompressed records, overlapped with "
                        "the tabulation of the previous chunk (0: decode the whole file first)")
    return p


def parse_write_groups(text):
    """The list of --write-groups, ``I[,I...]``, as a sorted tuple of group indices: any order, no repeats.  ValueError with
    the entry at fault for an empty entry, one that is not a decimal integer, a negative one or a repeat."""
    groups = []
    for entry in str(text).split(","):
        entry = entry.strip()
        if not entry:
            raise ValueError("an empty entry in %r (indices of groups.tsv, separated by commas)" % str(text))
        try:
            index = int(entry, 10)
        except ValueError:
            raise ValueError("%r is not an integer (indices of groups.tsv, not group names)" % entry) from None
        if index < 0:
            raise ValueError("group index %d is negative" % index)
        if index in groups:
            raise ValueError("group index %d is listed twice" % index)
        groups.append(index)
    return tuple(sorted(groups))


def check_write_groups(groups, n_groups):
    """... against the number of groups of the run, known once the header, the BED file or the thresholds are read."""
    for index in groups:
        if index >= n_groups:
            raise ValueError("--write-groups: group index %d is outside 0..%d (the run has %d groups, see groups.tsv)"
                             % (index, n_groups - 1, n_groups))


def parse_mask_ends(text):
    """--mask-ends, ``K5[,K3]``, as ``(k5, k3)``: one number means both ends.  ValueError for anything but one or two decimal
    integers of 0..255 that are not both 0."""
    entries = [entry.strip() for entry in str(text).split(",")]
    if len(entries) > 2:
        raise ValueError("%r has more than two numbers (K5[,K3])" % str(text))
    values = []
    for entry in entries:
        if not re.fullmatch(r"[0-9]+", entry):
            raise ValueError("%r is not a number of bases (K5[,K3], 0..255 each)" % entry)
        if int(entry) > 255:
            raise ValueError("%s is above 255 bases" % entry)
        values.append(int(entry))
    k5, k3 = values if len(values) == 2 else (values[0], values[0])
    if k5 == 0 and k3 == 0:
        raise ValueError("both ends are 0 bases: nothing to mask")
    return k5, k3


def _check_write_kept(parser, o):
    """The argument errors of --write-kept / --write-groups / --tag-group / --tag-pmd-score / --write-index / --mask-ends /
    --calmd."""
    if o.mask_what is not None and o.mask_ends is None:
        parser.error("--mask-what needs --mask-ends: it says what the windows of that option select")
    if o.mask_ends is not None:
        if o.write_kept is None:
            parser.error("--mask-ends needs --write-kept: it masks the records that file receives")
        try:
            o.mask_ends = parse_mask_ends(o.mask_ends)
        except ValueError as error:
            parser.error("--mask-ends: %s" % error)
        o.mask_what = o.mask_what or "all"
    if getattr(o, "calmd", False):
        if o.write_kept is None:
            parser.error("--calmd needs --write-kept: it recomputes NM and MD of the records that file receives")
        for option, tag in (("--tag-group", o.tag_group), ("--tag-pmd-score", o.tag_pmd_score)):
            if tag in ("NM", "MD"):
                parser.error("%s %s with --calmd: NM and MD are the two tags that option replaces" % (option, tag))
    if o.write_groups is not None:
        if o.write_kept is None:
            parser.error("--write-groups needs --write-kept: it chooses the groups whose records that file receives")
        if not o.grouping_options:
            parser.error("--write-groups needs a run with groups: one of " + groupings.OPTION_LIST)
        try:
            o.write_groups = parse_write_groups(o.write_groups)
        except ValueError as error:
            parser.error("--write-groups: %s" % error)
    for option, tag in (("--tag-group", o.tag_group), ("--tag-pmd-score", o.tag_pmd_score)):
        if tag is None:
            continue
        if o.write_kept is None:
            parser.error("%s needs --write-kept: it tags the records that file receives" % option)
        if not re.fullmatch(r"[A-Za-z][A-Za-z0-9]", tag):
            parser.error("%s %s: a tag is two characters, [A-Za-z][A-Za-z0-9]" % (option, tag))
    if o.tag_group is not None and not o.grouping_options:
        parser.error("--tag-group needs a run with groups: one of " + groupings.OPTION_LIST)
    if o.tag_pmd_score is not None and not o.by_pmd_score:
        parser.error("--tag-pmd-score needs --by-pmd-score: the score is the one that run computes")
    if o.tag_group is not None and o.tag_group == o.tag_pmd_score:
        parser.error("--tag-group and --tag-pmd-score name the same tag, %s: a record has a tag once" % o.tag_group)
    if getattr(o, "write_index", False) and o.write_kept is None:
        parser.error("--write-index needs --write-kept: it indexes the file that option writes")
    if o.write_kept is None:
        return
    if o.rescale_only or o.stats_only:
        parser.error("--write-kept belongs to the tabulation pass; neither --rescale-only nor --stats-only counts records")
    if not o.gpu_decode:
        parser.error("--write-kept is written by the device decode path: not with --host-decode")
    if o.gpus > 1:
        parser.error("--write-kept cannot be combined with --gpus %d: the ranks take alternate slabs of the input, and one "
                     "file has one order; use --gpus 1" % o.gpus)
    if o.downsample is not None and o.downsample >= 1:
        parser.error("--write-kept cannot be combined with -n %d: the reservoir of a fixed number of reads is the host's and "
                     "knows its sample at the end of the input only; a fraction (-n below 1) is drawn on the way" % int(o.downsample))
    if not Path(o.write_kept).absolute().parent.is_dir():
        parser.error("--write-kept %s: its directory does not exist" % o.write_kept)
    if o.filename is not None and not is_stream(o.filename):
        try:
            same = os.path.samefile(o.filename, o.write_kept)
        except OSError:
            same = False
        if same:
            parser.error("--write-kept %s is the input file: the run would overwrite what it reads" % o.write_kept)


DUPLICATE_ENDS = ("both", "5p")


def _check_remove_duplicates(parser, o):
    """The argument errors of --remove-duplicates / --duplicate-ends."""
    if o.duplicate_ends is not None and not o.remove_duplicates:
        parser.error("--duplicate-ends needs --remove-duplicates: it says which ends of a molecule that option compares")
    if not o.remove_duplicates:
        return
    o.duplicate_ends = o.duplicate_ends or "both"
    if o.rescale_only or o.stats_only:
        parser.error("--remove-duplicates belongs to the tabulation pass; neither --rescale-only nor --stats-only counts records")
    if not o.gpu_decode:
        parser.error("--remove-duplicates marks the records on the device decode path: not with --host-decode")
    if o.gpus > 1:
        parser.error("--remove-duplicates cannot be combined with --gpus %d: the ranks take alternate slabs of the input, and a "
                     "set of molecules per rank would miss the copies another rank has seen; use --gpus 1" % o.gpus)
    if o.downsample is not None and o.downsample >= 1:
        parser.error("--remove-duplicates cannot be combined with -n %d: the reservoir of a fixed number of reads is the host's; "
                     "a fraction (-n below 1) is drawn on the way, in front of the duplicates" % int(o.downsample))


def _check_depth(parser, o):
    """The argument errors of --depth / --depth-bedgraph / --depth-regions / --depth-thresholds."""
    if o.depth_bedgraph is not None and not o.depth:
        parser.error("--depth-bedgraph needs --depth: it writes the runs of the depth that option gathers")
    if o.depth_thresholds is not None and not o.depth_regions:
        parser.error("--depth-thresholds needs --depth-regions: it chooses the lines of that option's depth_thresholds.tsv")
    if o.depth_regions:
        if not o.depth:
            parser.error("--depth-regions needs --depth: it parts the depth that option gathers")
        if not (o.regions or o.region_groups):
            parser.error("--depth-regions needs --regions or --region-groups: the regions it parts the depth by")
        try:
            o.depth_thresholds = depth_files.parse_thresholds(o.depth_thresholds)
        except ValueError as error:
            parser.error(str(error))
    if not o.depth:
        return
    if o.rescale_only or o.stats_only:
        parser.error("--depth belongs to the tabulation pass; neither --rescale-only nor --stats-only counts records")
    if not o.gpu_decode:
        parser.error("--depth is gathered on the device decode path: not with --host-decode")
    if o.gpus > 1:
        parser.error("--depth cannot be combined with --gpus %d: the ranks take alternate slabs of the input, and the "
                     "accumulators of the ranks would have to be summed across the cards; use --gpus 1" % o.gpus)
    if o.downsample is not None and o.downsample >= 1:
        parser.error("--depth cannot be combined with -n %d: the reservoir of a fixed number of reads is the host's and knows "
                     "its sample at the end of the input only; a fraction (-n below 1) is drawn on the way" % int(o.downsample))
    if o.depth_bedgraph is not None:
        if not Path(o.depth_bedgraph).absolute().parent.is_dir():
            parser.error("--depth-bedgraph %s: its directory does not exist" % o.depth_bedgraph)
        if o.filename is not None and not is_stream(o.filename):
            try:
                same = os.path.samefile(o.filename, o.depth_bedgraph)
            except OSError:
                same = False
            if same:
                parser.error("--depth-bedgraph %s is the input file: the run would overwrite what it reads" % o.depth_bedgraph)


def _check_pileup(parser, o):
    """The argument errors of --pileup-sites and the --pileup-* options; the defaults filled in."""
    given = [name for name, value in (("--pileup-min-basequal", o.pileup_min_basequal), ("--pileup-mask-ends", o.pileup_mask_ends),
                                      ("--pileup-call", o.pileup_call), ("--pileup-seed", o.pileup_seed),
                                      ("--pileup-min-depth", o.pileup_min_depth),
                                      ("--pileup-single-strand-mode", o.pileup_single_strand_mode or None)) if value is not None]
    with_likelihoods = [name for name, value in (("--pileup-noqual-quality", o.pileup_noqual_quality), ("--pileup-beagle", o.pileup_beagle))
                        if value is not None]
    if with_likelihoods and not o.pileup_likelihoods:
        parser.error("%s need%s --pileup-likelihoods: the genotype likelihoods they belong to" % (" / ".join(with_likelihoods),
                                                                                                 "s" if len(with_likelihoods) == 1 else ""))
    if o.pileup_damage_positions is not None and o.pileup_damage_profile is None:
        parser.error("--pileup-damage-positions needs --pileup-damage-profile: the table whose positions it counts")
    if o.pileup_damage_profile is not None and not o.pileup_likelihoods:
        parser.error("--pileup-damage-profile needs --pileup-likelihoods: the genotype likelihoods whose error model it enters")
    if o.pileup_likelihoods and o.pileup_sites is None:
        parser.error("--pileup-likelihoods needs --pileup-sites: the list of sites the likelihoods are made at")
    if o.pileup_sites is None:
        if given:
            parser.error("%s need%s --pileup-sites: the list of sites the pileup is made at" % (" / ".join(given), "s" if len(given) == 1 else ""))
        return
    if o.rescale_only or o.stats_only:
        parser.error("--pileup-sites belongs to the tabulation pass; neither --rescale-only nor --stats-only counts records")
    if not o.gpu_decode:
        parser.error("--pileup-sites is gathered on the device decode path: not with --host-decode")
    if o.gpus > 1:
        parser.error("--pileup-sites cannot be combined with --gpus %d: the ranks take alternate slabs of the input, and the "
                     "counters of the ranks would have to be summed across the cards; use --gpus 1" % o.gpus)
    if o.downsample is not None and o.downsample >= 1:
        parser.error("--pileup-sites cannot be combined with -n %d: the reservoir of a fixed number of reads is the host's and knows "
                     "its sample at the end of the input only; a fraction (-n below 1) is drawn on the way" % int(o.downsample))
    o.pileup_min_basequal = 0 if o.pileup_min_basequal is None else o.pileup_min_basequal
    if not 0 <= o.pileup_min_basequal <= 93:
        parser.error("--pileup-min-basequal %d: a quality is 0..93" % o.pileup_min_basequal)
    if o.pileup_min_basequal and o.minqual and o.pileup_min_basequal > o.minqual:
        parser.error("--pileup-min-basequal %d is above --min-basequal %d: the decoder drops the qualities of a slab none of whose "
                     "bases is below --min-basequal, so a higher threshold cannot be applied beside it" % (o.pileup_min_basequal, o.minqual))
    try:
        o.pileup_mask_ends = pileup_files.parse_mask_ends(o.pileup_mask_ends)
    except ValueError as error:
        parser.error("--pileup-mask-ends: %s" % error)
    o.pileup_call = o.pileup_call or "random"
    o.pileup_seed = 0 if o.pileup_seed is None else o.pileup_seed
    if not 0 <= o.pileup_seed < 1 << 64:
        parser.error("--pileup-seed %d: an unsigned number of 64 bits" % o.pileup_seed)
    o.pileup_min_depth = 1 if o.pileup_min_depth is None else o.pileup_min_depth
    if not 1 <= o.pileup_min_depth < 1 << 31:
        parser.error("--pileup-min-depth %d: at least 1" % o.pileup_min_depth)
    try:
        with open(o.pileup_sites, "r") as handle:
            alleles = pileup_files.first_line_has_alleles(handle)
    except (OSError, UnicodeDecodeError) as error:
        parser.error("--pileup-sites %s: %s" % (o.pileup_sites, error))
    if alleles is None:
        parser.error("--pileup-sites %s holds no site" % o.pileup_sites)
    if o.pileup_single_strand_mode and not alleles:
        parser.error("--pileup-single-strand-mode needs Ref and Alt on every site: the lines of %s bring no alleles" % o.pileup_sites)
    if not o.pileup_likelihoods:
        return
    if o.minqual:
        parser.error("--pileup-likelihoods cannot be combined with -Q %d: under --min-basequal the decoder drops the quality column of "
                     "a slab none of whose bases is below the threshold, and the likelihoods need every base's quality; "
                     "--pileup-min-basequal sets a threshold for the sites" % o.minqual)
    o.pileup_noqual_quality = 30 if o.pileup_noqual_quality is None else o.pileup_noqual_quality
    if not 1 <= o.pileup_noqual_quality <= 93:
        parser.error("--pileup-noqual-quality %d: a quality of 1..93" % o.pileup_noqual_quality)
    if o.pileup_beagle is not None:
        if not alleles:
            parser.error("--pileup-beagle needs Ref and Alt on every site, the two alleles of its three genotypes: the lines of %s "
                         "bring no alleles" % o.pileup_sites)
        if not Path(o.pileup_beagle).absolute().parent.is_dir():
            parser.error("--pileup-beagle %s: its directory does not exist" % o.pileup_beagle)
        if o.filename is not None and not is_stream(o.filename):
            try:
                same = os.path.samefile(o.filename, o.pileup_beagle)
            except OSError:
                same = False
            if same:
                parser.error("--pileup-beagle %s is the input file: the run would overwrite what it reads" % o.pileup_beagle)
    if o.pileup_damage_profile is None:
        return
    if o.single_stranded:
        parser.error("--pileup-damage-profile cannot be combined with --single-stranded: in such a library both ends deaminate C>T, "
                     "and the rate of a base is a function of both its distances, which the profile's two rows per base do not give")
    if o.filename is not None and not is_stream(o.filename):
        try:
            same = os.path.samefile(o.filename, o.pileup_damage_profile)
        except OSError:
            same = False
        if same:
            parser.error("--pileup-damage-profile %s is the input file: a misincorporation.txt is expected" % o.pileup_damage_profile)
    o.pileup_damage_positions = pileup_files.GLD_DEFAULT_POSITIONS if o.pileup_damage_positions is None else o.pileup_damage_positions
    if not 1 <= o.pileup_damage_positions <= pileup_files.GLD_MAX_POSITIONS:
        parser.error("--pileup-damage-positions %d: 1..%d positions" % (o.pileup_damage_positions, pileup_files.GLD_MAX_POSITIONS))
    try:
        o.pileup_damage_profile_rows = pileup_files.read_damage_profile(o.pileup_damage_profile, o.pileup_damage_positions)
    except (OSError, UnicodeDecodeError) as error:
        parser.error("--pileup-damage-profile %s: %s" % (o.pileup_damage_profile, error))
    except pileup_files.ProfileError as error:
        parser.error("--pileup-damage-profile: %s" % error)


def parse_args(argv):
    parser = build_parser()
    o = parser.parse_args(argv)
    if o.plot_only or o.check_R_packages:
        parser.error("plotting is not part of this engine; run it with the reference on the emitted tables")
    if o.forward:                                                       # config.py:255-266: both set --termini
        o.termini = "5p"
    if o.reverse:
        o.termini = "3p"
    o.want_stats = o.stats or o.stats_only or o.rescale
    if o.want_stats:
        from .stats import StatsError, StatsOptions
        if o.no_stats:
            parser.error("--no-stats contradicts --stats / --stats-only / --rescale")
        if o.rescale_only:
            parser.error("--rescale-only works from an existing Stats_out_MCMC_correct_prob.csv; it runs no estimate")
        if o.stats_only and (o.stats or o.rescale):
            parser.error("--stats-only works from an existing folder; it excludes --stats and --rescale")
        try:
            o.stats_options = StatsOptions.from_args(o)
        except StatsError as error:
            parser.error(str(error))
        if o.seq_length > o.length and not o.stats_only:
            parser.error("--seq-length must not be greater than --length: the tables hold no position beyond it")
    from .sam import RecordFilter
    if o.min_read_length and o.max_read_length and o.min_read_length > o.max_read_length:
        parser.error("--min-read-length must not be greater than --max-read-length")
    o.record_filter = RecordFilter(o.min_mapq, o.require_flags, o.exclude_flags, o.min_read_length, o.max_read_length)
    if o.record_filter.active and (o.rescale_only or o.stats_only):
        parser.error("--min-mapq / --require-flags / --exclude-flags / --min-read-length / --max-read-length belong to the "
                     "tabulation pass; neither --rescale-only nor --stats-only counts records")
    # A run has one kind of groups (groupings.KINDS).  (--stats-only: see Kind.ignored_by_stats_only)
    live = [kind for kind in groupings.KINDS if not (o.stats_only and kind.ignored_by_stats_only)]
    o.grouping_options = [option for kind in groupings.KINDS for option in kind.given(o)]
    for kind in live:
        if kind.given(o, kind.companions) and not kind.given(o):
            parser.error("%s need%s %s" % (" / ".join(kind.companions), "s" if len(kind.companions) == 1 else "", " or ".join(kind.options)))
    kind = next((kind for kind in live if kind.given(o)), None)
    if kind is not None:
        if len(o.grouping_options) > 1:
            parser.error("%s exclude each other: a run has one kind of groups, chosen by one of %s"
                         % (" and ".join(o.grouping_options), groupings.OPTION_LIST))
        if o.rescale_only or o.stats_only:
            parser.error("%s belong%s to the tabulation pass; %s counts nothing"
                         % (" / ".join(kind.options), "s" if len(kind.options) == 1 else "", "--rescale-only" if o.rescale_only else "--stats-only"))
        try:
            kind.prepare(o)
        except ValueError as error:
            parser.error(str(error))
    _check_write_kept(parser, o)
    _check_remove_duplicates(parser, o)
    _check_depth(parser, o)
    _check_pileup(parser, o)
    if o.stats_only:
        if not o.folder:
            parser.error("--folder required when using --stats-only")
        if not o.jukes_cantor and not (o.folder / "dnacomp_genome.csv").is_file() and not o.ref:
            parser.error("--stats-only needs dnacomp_genome.csv in the folder, or --reference to make it from")
        o.no_stats = False
        return o
    if o.rescale_only and not o.folder:
        parser.error("--folder required when using --rescale-only")
    if not o.filename:
        parser.error("--input SAM/BAM file not specified")
    if is_stream(o.filename):
        # (a stream is read once, by one process, front to back)
        if o.gpus > 1:
            parser.error("--gpus %d cannot read its input from stdin or a pipe: every rank opens the input itself; "
                         "write it to a file, or use --gpus 1" % o.gpus)
        if o.rescale_only:
            parser.error("--rescale-only cannot read its input from stdin or a pipe (it reads the file more than once); "
                         "write it to a file")
        if o.rescale:
            parser.error("Cannot build model and rescale in one run when input is a pipe")          # main.py:133-136
    if not o.ref:
        parser.error("--reference FASTA file not specified")
    if o.downsample is not None:
        if o.downsample <= 0:
            parser.error("-n/--downsample must be a positive value")
        elif o.downsample >= 1:
            o.downsample = int(o.downsample)
    if o.ymax <= 0 or o.ymax > 1:
        parser.error("--ymax (-b) must be an real number beetween 0 and 1")
    if o.refplot > o.around:
        parser.error("--refplot (-b) must be less than --around (-a)")
    if o.readplot > o.length:
        parser.error("--readplot (-m) must be less than --length (-l)")
    if not o.folder:
        o.folder = Path(o.filename.stem + ".mapDamage")
    o.folder.mkdir(parents=True, exist_ok=True, mode=0o750)
    o.no_stats = not o.want_stats
    if not o.rescale_out and (o.rescale or o.rescale_only):
        o.rescale_out = o.folder / (o.filename.stem + ".rescaled.bam")
    if o.rescale_length_3p is None:
        o.rescale_length_3p = o.seq_length
    elif not (0 <= o.rescale_length_3p <= o.seq_length):
        parser.error("--rescale-length-3p must be less than or equal to --seq-length and greater than zero")
    if o.rescale_length_5p is None:
        o.rescale_length_5p = o.seq_length
    elif not (0 <= o.rescale_length_5p <= o.seq_length):
        parser.error("--rescale-length-5p must be less than or equal to --seq-length and greater than zero")
    return o


def rescale_qual(options):
    """Mirror of rescale.rescale_qual (mapdamage/rescale.py:368-383) for --rescale-only."""
    from .rescale import RescaleError, RescaleModel, rescale_bam
    from .sam import BamStream
    logger = logging.getLogger(__name__)
    logger.info("Rescaling BAM: '%s' -> '%s'", options.filename, options.rescale_out)
    start = time.time()
    try:
        model = RescaleModel.from_csv(options.folder / "Stats_out_MCMC_correct_prob.csv",
                                      options.rescale_length_5p, options.rescale_length_3p)
        # the header only (the records are streamed by rescale_bam).  The reference's --rescale-only branch
        # (main.py:121-124) goes straight to rescale_qual without the .fai / dictionary checks of the tabulation
        # pass: a sequence the FASTA lacks, or holds at another length, only matters when a record maps there
        # (fetch fails at that read) — here such a record is a bad record when the kernel meets it.
        with BamStream(options.filename) as probe:
            header = probe.header
        ref = reference_for_bam(options.ref, header.references, missing_ok=True)
        for name, length, have in zip(header.references, header.lengths, ref.lengths):
            if have != length:
                logger.warning("FASTA sequence %r is %s; the BAM header says %i bp — records mapped to it may fail",
                               name, "missing" if not have else "%i bp" % have, length)
        with DamageEngine([("*", "*")], options.length, options.around, 0, device=options.device) as engine:
            summary = None
            if options.gpu_decode and not options.host_deflate and _device_path_applies(options, sam_text=False):
                # the records never on the host: inflated, rescaled, written back and deflated in HBM
                from .rescale import rescale_bam_on_device
                from .sam import GpuDecodeUnsupported
                try:
                    summary, counts = rescale_bam_on_device(engine, ref, options.filename, options.rescale_out, model)
                except (GpuDecodeUnsupported, ValueError, MdxError) as error:
                    # (never silent; the host decoder reads the whole file again and words the errors as the reference does)
                    logger.warning("GPU decode path gave up: %s; rescaling through the host decoder (the whole file again)", error)
                    engine.reset()
                    summary = None
            if summary is None:
                summary, counts = rescale_bam(engine, ref, options.filename, options.rescale_out, model,
                                              device_deflate=not options.host_deflate)
    except RescaleError as error:
        logger.error("%s", error)
        return 1
    if counts["inward_pairs"] or counts["improper_pairs"]:
        logger.warning("Processed %i paired reads, assumed to be non-overlapping, facing inwards and correctly "
                       "paired; %i of these were excluded as improperly paired.",
                       counts["inward_pairs"] + counts["improper_pairs"], counts["improper_pairs"])
    if counts["without_qualities"]:
        logger.warning("Skipped %i reads without quality scores", counts["without_qualities"])
    for line in summary.log_lines():                                     # rescale.py:361-362
        logger.info("%s", line)
    logger.debug("Rescaling completed in %f seconds", time.time() - start)
    return 0


def _base_frequencies(options, ref, n_contig, device):
    """A, C, G, T of ``dnacomp_genome.csv`` (main.py:96-103, 248-250): read when the folder holds the file, otherwise counted
    on the device from the reference and written.  None with --jukes-cantor (main.r:33-35)."""
    from . import composition
    from .stats import read_base_freqs
    path = options.folder / "dnacomp_genome.csv"
    if not path.is_file() or ref is not None:
        if ref is None:
            # (--stats-only: every sequence of the FASTA, in the order of its index)
            if not is_plain_gzip(options.ref):
                ensure_fasta_index(options.ref)
            names = list(read_fasta_index(str(options.ref) + ".fai"))
            ref, n_contig = reference_for_bam(options.ref, names), len(names)
        with DamageEngine([("*", "*")], options.length, options.around, 0, device=device) as engine:
            engine.set_reference(ref)
            composition.write_base_comp(engine.genome_composition(n_contig), path)
    return None if options.stats_options.jukes_cantor else read_base_freqs(path)


def _group_has_data(folder):
    """The part of check_table_and_warn_if_dmg_freq_is_low that refuses a table (statistics.py), without its log lines."""
    from .statistics import _position_one_totals
    try:
        totals = _position_one_totals(folder / "misincorporation.txt")
    except (OSError, KeyError, ValueError, IndexError):
        return False
    return totals is not None and totals[("5p", "C")] != 0 and totals[("3p", "G")] != 0


def bayesian_estimates(options, logger, ref=None, n_contig=0, device=0):
    """The estimate of the folder's tables and of every group directory beside them (<a kind's directory>/<index>:
    groupings.KINDS), all chains in one launch: mapdamage/rscript.py:70-100 without R.  Returns the exit code."""
    from .stats import StatsError, estimate_folders
    start = time.time()
    try:
        acgt = _base_frequencies(options, ref, n_contig, device)
        folders, chains = [options.folder], [options.stats_chain]
        for sub in (kind.directory for kind in groupings.KINDS):
            if not (options.folder / sub / "groups.tsv").is_file():
                continue
            index = 0
            while (options.folder / sub / str(index) / "misincorporation.txt").is_file():
                group = options.folder / sub / str(index)
                if _group_has_data(group):
                    folders.append(group)
                    chains.append(index + 1)
                else:
                    logger.info("Group %d of %s: too few reads for the Bayesian estimate (no C at the first 5' position or no "
                                "G at the first 3' position); skipped", index, sub)
                index += 1
        estimate_folders(folders, acgt, options.stats_options, chains, device, logger)
    except (StatsError, MdxError, OSError, ValueError) as error:
        logger.error("Bayesian estimate failed: %s", error)
        return 1
    logger.debug("Bayesian estimates made in %f seconds", time.time() - start)
    return 0


def _sum_words(words, device):
    """uint64 words summed over the ranks (``device``: where the backend wants them; None: the host)."""
    import torch
    from .distributed import allreduce_words
    words = torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64).copy())
    return allreduce_words(words if device is None else words.to(device)).cpu().numpy().view(np.uint64)


class _Ranks:
    """The ranks of a multi-GPU run (mapdamage/main.py:165-217 sharded by record): one process per GPU under
    torch.distributed; rank r of W takes the slabs (device decode) or the shard of every chunk (host decode) that are
    its own, nothing is exchanged until the tables are summed."""

    def __init__(self, options):
        import os
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.backend = options.dist_backend
        self.device = options.device
        if self.world > 1:
            import torch
            import torch.distributed as dist
            if not options.share_gpu:
                self.device = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(self.device)
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if not dist.is_initialized():
                if self.backend == "nccl":
                    dist.init_process_group("nccl", device_id=torch.device("cuda", self.device))
                else:
                    dist.init_process_group("gloo")

    def finish(self, engine, error=None):
        """The tables of the whole run, on every rank.  ``error``: what this rank's part of the run died of, if it did —
        the ranks agree on it before any collective, the failing one re-raises it, the others raise RuntimeError."""
        if self.world == 1:
            if error is not None:
                raise error
            return engine.finish()
        from . import distributed
        if self.backend == "nccl":
            import torch
            dev = torch.device("cuda", self.device)
            distributed.agree_on_error(error, dev)
            return self._strata(engine, distributed.reduce_engine_tables(engine, dev), dev)
        own = None
        if error is None:
            try:
                own = engine.finish()
                if engine.groups is not None:
                    own = own.strata
            except (BadReadError, MdxError) as exc:
                error = exc
        distributed.agree_on_error(error)
        return self._strata(engine, distributed.reduce_tableset(own, engine.lgd_max), None)

    @staticmethod
    def _strata(engine, block, device):
        """The summed block of a stratified engine (its layout is the one of any block: ``nlib`` tables in stratum order)
        split by group, with the kept reads per stratum summed over the ranks as well."""
        if engine.groups is None:
            return block
        from .tables import StratifiedTables
        out = StratifiedTables.from_block(block, engine.base_libraries, engine.groups, _sum_words(engine.strata_kept(), device))
        kind = groupings.BY_NAME[engine.strata_kind]
        words = kind.rank_words(engine)
        if words is not None:
            kind.take_rank_words(out, _sum_words(words, device))
        return out

    def sum_counts(self, counts):
        """The record filters' counts (uint64[6]) summed over the ranks, as the kept reads per stratum are."""
        counts = np.ascontiguousarray(counts, np.uint64)
        if self.world == 1:
            return counts
        import torch
        return _sum_words(counts, torch.device("cuda", self.device) if self.backend == "nccl" else None)

    def close(self):
        if self.world > 1:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.barrier()
                dist.destroy_process_group()


def launch_command(argv, gpus):
    """The command ``--gpus N`` re-executes itself under: one rank per GPU of this node."""
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    keep = [a for a in argv if a != "--print-launch"]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "mapdamage_amd"] + keep


def reference_strata(options, references, lengths=None):
    """(group names, payload) of the run's kind of groups (``groupings.KINDS``: what the kind's ``apply`` hands the engine)
    from the options and the header's sequences and their ``lengths``, or None."""
    kind = groupings.kind_of(options)
    return None if kind is None else kind.payload(options, references, lengths)


def _make_engine(options, libraries, device):
    """The run's engine; with a grouping option one table set per (library, group) — the input routes hand it the same
    batches either way."""
    strata = getattr(options, "strata", None)
    engine = DamageEngine(libraries, options.length, options.around, options.minqual, device=device,
                          groups=None if strata is None else strata[0])
    if strata is not None:
        try:
            groupings.kind_of(options).apply(engine, strata[1], options)
        except Exception:
            engine.close()
            raise
    return engine


def _report_record_filters(options, counts, logger, first):
    """The INFO line and record_filters.tsv of a run with record filters (rank 0; ``counts``: summed over the ranks)."""
    if not first:
        return
    f = options.record_filter
    n, a, b, c, d, e = (int(x) for x in counts)
    logger.info("Record filters: %d records read; dropped: %d require-flags, %d exclude-flags, %d MAPQ < %d, %d shorter than %d, "
                "%d longer than %d", n, a, b, c, f.min_mapq, d, f.min_length, e, f.max_length)
    lines = ["filter\tvalue\trecords_dropped",
             "require-flags\t0x%X\t%d" % (f.require_flags, a), "exclude-flags\t0x%X\t%d" % (f.exclude_flags, b),
             "min-mapq\t%d\t%d" % (f.min_mapq, c), "min-read-length\t%d\t%d" % (f.min_length, d),
             "max-read-length\t%d\t%d" % (f.max_length, e), "records-read\t\t%d" % n,
             "records-passed\t\t%d" % (n - a - b - c - d - e)]
    (options.folder / "record_filters.tsv").write_text("\n".join(lines) + "\n")


def _tabulate_on_host(options, reader, ref, libraries, logger, ranks, carry=None):
    """The records decoded on the host (native BGZF/BAM decoder or SAM text), uploaded batch by batch.
    ``carry``: (engine, resume position, records counted so far, --downsample generator or None) of a device decode that
    gave up part of the way: the same engine — its tables hold the slabs already counted — goes on with the rest of the
    file (a stream's draws with the run's one generator, where the device path left it)."""
    import contextlib
    with contextlib.ExitStack() as stack:
        if carry is None:
            engine = stack.enter_context(_make_engine(options, libraries, ranks.device))
            engine.set_reference(ref)
            n_reads, resume, rand = 0, None, None
        else:
            engine, resume, n_reads, rand = carry[:4]
            stack.enter_context(engine)
        warned_about_quals = False
        error = None
        # a BAM file arrives in chunks (bounded host memory; chunk k+1 is decoded while chunk k is tabulated)
        for batch in reader.iter_batches(resume=resume, rand=rand):
            if options.minqual and not warned_about_quals and batch.n:
                # main.py:185-192: the first iterated read without qualities (`not read.qual`: absent or
                # empty) triggers the warning, once
                lens = np.diff(batch.seq_off.astype(np.int64))
                first = np.minimum(batch.seq_off[:-1].astype(np.int64), max(0, batch.seq.shape[0] - 1))
                if batch.qual is None or bool(((lens == 0) | (batch.qual[first] == 0xFF)).any()):
                    logger.warning("Reads without PHRED scores found; cannot filter by --min-basequal")
                    warned_about_quals = True
            if options.minqual:
                # records none of whose qualities is below the threshold cannot be masked: the kernel skips their
                # quality windows; a chunk without a single maskable base goes through the unmasked kernel
                batch, nothing_to_mask = mark_unmaskable(batch, options.minqual)
                if nothing_to_mask:
                    batch = dataclasses.replace(batch, qual=None)
            # the slices of a chunk are enqueued one behind the other — the copy of slice k+1 runs under the kernel of
            # slice k — and the chunk is waited for once; a bad record comes back with its index among all records
            # iterated so far (the reference would name the read)
            # (several ranks: every rank decodes the chunk — the host decoder is one stream of records — and counts its
            # own contiguous shard of it)
            from .distributed import shard_bounds
            s_lo, s_hi = shard_bounds(batch.n, ranks.rank, ranks.world)
            try:
                for lo in range(s_lo, s_hi, options.batch_reads):
                    engine.tabulate(batch.slice(lo, min(s_hi, lo + options.batch_reads), copy=False), sync=False,
                                    record_base=n_reads + lo)
                engine.sync()
            except (BadReadError, MdxError) as exc:
                if ranks.world == 1:
                    raise
                error = exc
                break
            n_reads += batch.n
        # the record filters' counts: the reader's (where a host decoder took over part of the way, on top of the device
        # path's); several ranks decode the same chunks, rank 0 speaks for all
        counts = reader.filter_counts.copy()
        if carry is not None and len(carry) > 4:
            counts += carry[4]
        options.filter_counts = counts if ranks.rank == 0 else np.zeros(6, np.uint64)
        tables = ranks.finish(engine, error)
    return tables


def _device_path_applies(options, world=1, sam_text=True):
    """BAM files on disk; --downsample to a fraction too (the draws are made on the host from the flag column of every slab,
    reader.py:134-146) unless several ranks share the file (a rank steps over the slabs of the others without seeing their
    flags, and the stream of draws is the whole file's); a fixed number of reads is reservoir sampling over the whole file
    (reader.py:148-164): the host's.  SAM text (``sam_text``: the tabulation pass, not --rescale-only) for one rank, plain or
    bgzip-compressed; a plain gzip file's members have no blocks to share out among the device's lanes: the host's."""
    from .sam import BAM, SAM_GZIP, input_format
    # (stdin and pipes as files: through the run's one Source, options.source — a stream is never opened twice)
    source = getattr(options, "source", None)
    if source is None and is_stream(options.filename):
        return False
    kind = getattr(options, "input_kind", None)
    if kind is None:        # (sniffed once per run)
        kind = options.input_kind = input_format(source if source is not None else options.filename)
    if kind == SAM_GZIP:
        return False
    bam = kind == BAM
    return (bam or (sam_text and world == 1)) and (options.downsample is None or (options.downsample < 1 and world == 1))


def _expected_records(options, reader):
    """What sizes the first table of --remove-duplicates: a regular file's bytes over 48 (a short read with its qualities
    compresses to 40 to 70 bytes in BAM), 0 — a small table that grows — for a stream.  Only the number of times the table
    grows, and the slots it ends with, depend on it."""
    source = getattr(reader, "source", None)
    if source is not None and source.is_stream:
        return 0
    try:
        return os.path.getsize(options.filename) // 48
    except (OSError, TypeError):
        return 0


def _slab_bytes(options, world):
    """Compressed bytes per slab of the device decode path: a quarter of --chunk-mb (a slab of compressed bytes inflates to
    about four times its size) — 256 MiB at the default.  (Rounds 4-5 gave a single rank slabs of 1 GiB, for their fixed
    costs; since the slabs run as a pipeline of two — the device goes from one slab's inflate straight into the next one's —
    more, smaller slabs fill it better, and the pinned buffer of the host's share is a quarter of the size.)"""
    import os
    slab = max(1 << 20, int(options.chunk_mb * (1 << 20)) // 4) if options.chunk_mb else 256 << 20
    if os.environ.get("MDX_GBAM_SLAB_BYTES"):      # (tests: several slabs out of a small file whatever --chunk-mb says)
        slab = max(1 << 16, int(os.environ["MDX_GBAM_SLAB_BYTES"]))
    return slab


class _KeptOutput:
    """--write-kept on the device decode path: the BAM file under a temporary name in its own directory — the input's header
    first, then every slab's kept records as the device hands them over (``sam.GpuBamStream.write_kept``), written by the
    writer's thread under the next slab's decode and tabulation —, moved into place by ``commit`` behind the end-of-file marker.
    Leaving the ``with`` block any other way removes the temporary file."""

    def __init__(self, options, engine, stream):
        from .sam import BgzfWriter, bam_header_bytes
        self.path = Path(options.write_kept)
        self.tmp = self.path.with_name("%s.%d.tmp" % (self.path.name, os.getpid()))
        self.groups = options.write_groups
        self.group_tag, self.score_tag = getattr(options, "tag_group", None), getattr(options, "tag_pmd_score", None)
        tagged = self.group_tag is not None or self.score_tag is not None
        self.n_groups = len(options.strata[0]) if self.groups is not None or tagged else 0
        self.stream, self.folder = stream, options.folder
        self.records = self.raw_bytes = 0
        # (--write-index: PATH.bai, the name samtools looks for, under a temporary name of its own until the BAM is in place)
        self.index = None
        if getattr(options, "write_index", False):
            from .bai import BaiAssembler
            self.index = BaiAssembler(stream.header.lengths)
            self.index_path = Path(str(self.path) + ".bai")
            self.index_tmp = self.index_path.with_name("%s.%d.tmp" % (self.index_path.name, os.getpid()))
            self.index_prev = (-1, -1)
        # (--mask-ends: the stream masks every slab it writes from here on, and counts)
        self.mask = getattr(options, "mask_ends", None)
        if self.mask is not None:
            self.mask_what, self.mask_single = options.mask_what, bool(options.single_stranded)
            stream.set_kept_mask(self.mask[0], self.mask[1], self.mask_what, self.mask_single)
        # (--calmd: NM and MD of every slab it writes from here on recomputed, and counted)
        self.calmd = bool(getattr(options, "calmd", False))
        if self.calmd:
            stream.set_kept_md(True)
        self.writer = BgzfWriter(self.tmp, engine=engine)
        try:
            self.writer.write(bam_header_bytes(stream.header))
        except BaseException:
            self._remove()
            raise

    def add(self, view):
        """The slab's kept records: right behind ``engine.tabulate_view(view)`` — the flags are final, the key column is the
        view's."""
        self.writer.flush()             # (the one output array is the writer thread's until its write is done)
        members, n, raw = self.stream.write_kept(view, self.groups, self.n_groups, self.group_tag, self.score_tag)
        if self.index is not None and n:
            from .bai import member_sizes
            runs, self.index_prev = self.stream.kept_index(self.raw_bytes, self.index_prev, n)
            self.index.add_slab(self.raw_bytes, self.writer.bytes_handed, member_sizes(members), raw, runs)
        self.records += n
        self.raw_bytes += raw
        if len(members):
            self.writer.write_members(members)

    def commit(self, logger):
        index = None
        masked = self.stream.kept_mask_counts() if self.mask is not None else None
        recomputed = self.stream.kept_md_counts() if self.calmd else None
        if self.index is not None:
            index = self.index.finish(self.stream.kept_index_linear())
            self.index_tmp.write_bytes(index)
        self.writer.close()             # (the queued writes, then the end-of-file marker)
        self.writer = None
        os.replace(self.tmp, self.path)
        if index is not None:
            os.replace(self.index_tmp, self.index_path)
        which = "all" if self.groups is None else ",".join(str(g) for g in self.groups)
        tags = ["%s:S group" % self.group_tag] if self.group_tag is not None else []
        tags += ["%s:f PMD score" % self.score_tag] if self.score_tag is not None else []
        logger.info("Wrote %d records to %s (groups: %s)%s", self.records, self.path, which, "; tags: " + ", ".join(tags) if tags else "")
        (self.folder / "write_kept.tsv").write_text("path\tgroups\trecords\tuncompressed_bytes\n%s\t%s\t%d\t%d\n"
                                                    % (self.path, which, self.records, self.raw_bytes))
        if masked is not None:
            logger.info("Masked %d bases in %d of %d written records (5p %d, 3p %d: %s)", masked[1], masked[0], self.records,
                        self.mask[0], self.mask[1], self.mask_what)
            (self.folder / "mask_ends.tsv").write_text("path\tk5\tk3\twhat\tsingle_stranded\trecords\tbases\n%s\t%d\t%d\t%s\t%d\t%d\t%d\n"
                                                       % (self.path, self.mask[0], self.mask[1], self.mask_what, int(self.mask_single),
                                                          masked[0], masked[1]))
        if recomputed is not None:
            logger.info("Recomputed NM and MD of %d of %d written records (%d left as they are)", recomputed[0], self.records, recomputed[1])
            (self.folder / "calmd.tsv").write_text("path\trecords\trecomputed\tskipped\thad_tags\n%s\t%d\t%d\t%d\t%d\n"
                                                   % (self.path, self.records, recomputed[0], recomputed[1], recomputed[2]))
        if index is not None:
            logger.info("Wrote index %s (%d references with records, %d chunks)", self.index_path, self.index.n_references, self.index.n_chunks)

    def _remove(self):
        if self.writer is not None:
            try:
                self.writer.abandon()
            except Exception:
                pass
            self.writer = None
        for tmp in (self.tmp,) + ((self.index_tmp,) if self.index is not None else ()):
            try:
                tmp.unlink()
            except OSError:
                pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._remove()          # (nothing to remove behind commit)


def _tabulate_on_device(options, reader, ref, libraries, logger, ranks, stages):
    """--gpu-decode: the file inflated, unpacked and counted on the GPU.  Returns (tables, None), or (None, carry) when
    the path does not apply or has given up — the caller decodes on the host, which also words the errors the way the
    reference does: the whole file (carry None), or, when the device path failed on a slab it had not begun to count,
    the rest of it with the same engine (``_tabulate_on_host``'s ``carry``)."""
    import contextlib
    from .sam import GpuBamStream, GpuDecodeUnsupported, GpuSamStream
    # a stream (stdin, a pipe) is read once: a host decoder that takes over goes on where the device path stopped, never
    # from the start
    streaming = reader.source is not None and reader.source.is_stream
    # SAM text: parsed on the device as well (sam.GpuSamStream); a stream of it is taken up by the host parser from the first
    # line of the slab that failed — also for a bad record or read group, so that the host words the error (the slab handed
    # out last stays in the stream until the next one is asked for: each slab is synchronised before the next)
    sam_text = not reader.is_bam
    sam_stream = sam_text and streaming
    if not _device_path_applies(options, ranks.world):
        logger.debug("the GPU decode path does not apply to this run; decoding on the host")
        return None, None
    import random
    downsample_rand = random.Random(options.downsample_seed)
    if options.merge_libraries:
        readgroups, lib_default = [], 0
    else:
        readgroups = [(rg, libraries.index(lib)) for rg, lib in reader._readgroups.items()]
        lib_default = None
    engine = _make_engine(options, libraries, ranks.device)
    stages.mark("engine")
    # (--by-pmd-score: the key reads the qualities beside the nibbles the packed kernel counts from)
    by_pmd = bool(getattr(options, "by_pmd_score", False))
    # (--write-kept: BAM input, one rank — parse_args and main have seen to it)
    write_kept = getattr(options, "write_kept", None) is not None and not sam_text
    # (--remove-duplicates: BAM input, one rank, as for --write-kept; the set of molecules lives on the device)
    dedup = bool(getattr(options, "remove_duplicates", False)) and not sam_text
    # (--depth: BAM input, one rank, likewise; the accumulator lies over the resident reference)
    depth = bool(getattr(options, "depth", False)) and not sam_text
    # (--pileup-sites: likewise; the sites and their counters are resident beside the reference)
    pileup = getattr(options, "pileup_sites_list", None) if not sam_text else None
    likelihoods = pileup is not None and bool(getattr(options, "pileup_likelihoods", False))
    pileup_qual = pileup is not None and (options.pileup_min_basequal > 0 or likelihoods)
    carry = None
    try:
        engine.set_reference(ref)
        if dedup:
            engine.dedup_begin(options.duplicate_ends, _expected_records(options, reader))
        if depth:
            engine.depth_begin()
        if pileup is not None:
            engine.pileup_begin(pileup.pos, pileup.off, pileup.alleles, min_basequal=options.pileup_min_basequal,
                                mask_ends=options.pileup_mask_ends, call=options.pileup_call, seed=options.pileup_seed,
                                min_depth=options.pileup_min_depth, single_strand=options.pileup_single_strand_mode)
            profile = getattr(options, "pileup_damage_profile_rows", None)
            if likelihoods and profile is not None:
                engine.pileup_likelihoods_damage_begin(pileup_files.damage_likelihood_table(profile), options.pileup_noqual_quality)
            elif likelihoods:
                engine.pileup_likelihoods_begin(pileup_files.likelihood_table(), options.pileup_noqual_quality)
        stages.mark("reference resident")
        warned_about_quals = False
        error = None
        slab = _slab_bytes(options, ranks.world)
        warm = getattr(options, "warm_thread", None)
        if warm is not None:
            warm.join()         # (the pinned buffer it leaves behind is the one the first slab takes)
        stages.mark("warm-up joined")
        with (GpuSamStream if sam_text else GpuBamStream)(
                engine, reader.source if reader.source is not None else options.filename, readgroups=readgroups,
                lib_default=lib_default, chunk_bytes=slab, want_qual=options.minqual != 0 or by_pmd or pileup_qual, min_basequal=options.minqual,
                packed=True if by_pmd or pileup_qual else None, record_filter=options.record_filter) as stream, \
                (_KeptOutput(options, engine, stream) if write_kept else contextlib.nullcontext()) as kept_out:
            # (several ranks: rank r decodes the slabs r, r + W, ... and steps over the others)
            slab, n_reads, n_kept = 0, 0, 0
            try:
                while True:
                    mine = slab % ranks.world == ranks.rank
                    slab += 1
                    if not mine:
                        if not stream.skip():
                            break
                        continue
                    if sam_stream:
                        slab_start, kept_before, rand_state = stream.tell(), n_kept, downsample_rand.getstate()
                        counts_before = stream.filter_counts()
                    try:
                        view = stream.next_view()
                    except ValueError:
                        # the decode of a slab failed before any of its records was counted: everything in front of it
                        # is in the engine's tables, and the host decoder can go on from the slab's first record
                        if ranks.world == 1:
                            engine.sync()
                            where = stream.tell()
                            # (resuming needs the chunked host decoder, reader.iter_batches(resume=...): with --chunk-mb 0
                            # the host path reads the file in one piece, so the whole file is counted again)
                            # (... and --downsample: the host decoder starts its stream of draws at the file's first record)
                            # (a stream cannot be read again: the host decoder takes it up at that slab, the first one too,
                            # and the draws go on with the run's one generator)
                            if where is not None and reader._chunks is not None and (
                                    streaming or (slab > 1 and options.downsample is None)):
                                carry = (engine, where, n_reads, downsample_rand if options.downsample is not None else None)
                            elif where is not None and sam_stream:
                                carry = (engine, where, n_kept, downsample_rand if options.downsample is not None else None)
                            if carry is not None:
                                # (the counts of the slabs in front.  A SAM slab that is given up has added nothing; a BAM slab
                                # that failed behind its unpack launch — a block's CRC32 — may have added to the reasons: the
                                # host decoder ends on that block's error, and the counts are never written)
                                carry += (stream.filter_counts(),)
                        raise
                    if view is None:
                        break
                    if options.downsample is not None:
                        # reader.py:134-146: one draw per record the flag filter keeps, in file order, from the run's one
                        # generator; the records that leave get a bit the kernel's flag filter drops
                        flags = stream.view_flags(view)
                        kept = np.nonzero((flags & FLAG_FILTER) == 0)[0]
                        stay = draw_uniform(downsample_rand, len(kept)) < options.downsample
                        flags[kept[~stay]] |= 0x200
                        stream.set_view_flags(view, flags)
                        # (main.py:185-192 warns about a read without qualities that the loop MEETS — one that survived the draws:
                        # the decoder marks the records that have qualities, include/mdx.h MDX_FLAG_HAS_QUAL)
                        if options.minqual and not warned_about_quals and bool(((flags[kept[stay]] & 0x4000) == 0).any()):
                            logger.warning("Reads without PHRED scores found; cannot filter by --min-basequal")
                            warned_about_quals = True
                    elif options.minqual and not warned_about_quals and stream.missing_qualities():
                        logger.warning("Reads without PHRED scores found; cannot filter by --min-basequal")
                        warned_about_quals = True
                    if dedup:
                        # (behind the draws, in front of the count: the later copies leave with 0x400, and everything from
                        # here on — the kernels' flag filter, the groups' keys, --write-kept — sees the final flags)
                        engine.dedup_mark(view)
                    if depth:
                        # (the final flags: behind the filters, the draws and the duplicates' marks)
                        engine.depth_add(view)
                    if pileup is not None:
                        engine.pileup_add(view)
                    engine.tabulate_view(view, record_base=n_reads)
                    if kept_out is not None:
                        kept_out.add(view)
                    if sam_stream:
                        try:
                            engine.sync()
                        except BadReadError:
                            downsample_rand.setstate(rand_state)
                            carry = (engine, slab_start, kept_before, downsample_rand if options.downsample is not None else None,
                                     counts_before)
                            raise
                        # (the records the host decoder would have counted: its record numbers go on from there)
                        kept = stream.view_flags(view) if options.downsample is None else flags
                        n_kept += int(((kept & FLAG_FILTER) == 0).sum())
                    n_reads += int(view.n_reads)
                engine.sync()
                stages.mark("decode and tabulate")
                if stream.fixups():
                    logger.debug("device decode: %d BGZF blocks rescanned from the record their predecessor's chain ended on", stream.fixups())
            except (BadReadError, ValueError, MdxError) as exc:
                if ranks.world == 1:
                    raise
                error = exc         # (the ranks agree on it in finish(): all of them take the host path then)
            if error is None:
                options.filter_counts = stream.filter_counts()
            tables = ranks.finish(engine, error)
            if dedup:
                options.duplicates = (engine.dedup_counts(), engine.dedup_histogram(), engine.dedup_info())
            if depth:
                options.depth_result = (list(ref.names), [int(x) for x in ref.lengths]) + engine.depth_finish() + (
                    engine.depth_runs() if options.depth_bedgraph is not None else None, engine.depth_info())
                if getattr(options, "depth_regions", False):
                    options.depth_regions_result = engine.depth_regions()
            if pileup is not None:
                options.pileup_result = (list(ref.names),) + engine.pileup_finish() + (engine.pileup_info(),)
                if likelihoods:
                    options.pileup_likelihoods_result = engine.pileup_likelihoods_finish(with_sums=False)[1:]
            if kept_out is not None:
                kept_out.commit(logger)
        # (the stream is closed first: mdx_gbam_close hands its arena back to the context, which must still be alive)
        engine.close()
        return tables, None
    except (KeptTagClash, KeptIndexError):
        # (--tag-group / --tag-pmd-score: a record has the tag already; --write-index: a written record out of order or out of
        # BAI's reach — the run's error, no other decoder would do better)
        engine.close()
        raise
    except GpuDecodeUnsupported as error:
        reason = "file layout the device path does not take (MDX_ERR_UNSUPPORTED): %s" % error
    except BadReadError as error:
        # a record the reference cannot process, or one without a usable read group: the host path names it — but a stream,
        # which the host decoder cannot read again up to that record: the device path's error stands
        if streaming and not sam_stream:
            engine.close()
            raise
        reason = "a record the device path cannot count (MDX_ERR_BAD_READ, record %d)" % error.read_index
        if not sam_stream:
            carry = None
    except (ValueError, MdxError) as error:
        # a damaged file (the host decoder finds the same damage and words the error), or the device path out of
        # memory: either way the host path has the last word
        reason = "%s (libmdx code %s)" % (error, getattr(error, "code", "n/a"))
    except RuntimeError as error:
        # (several ranks: another rank's part of the file failed — every rank takes the host path, like that one)
        reason = str(error)
    # never silent: a regression of the device path must not show up as nothing but a slow run
    options.gpu_decode_fallbacks = getattr(options, "gpu_decode_fallbacks", 0) + 1
    if write_kept or dedup or depth or pileup is not None:
        # (no route through the host decoder: the run ends, main says why)
        engine.close()
        logger.warning("GPU decode path gave up: %s", reason)
        return None, None
    if carry is None:
        engine.close()
        logger.warning("GPU decode path gave up: %s; decoding on the host (the whole file again)", reason)
    else:
        logger.warning("GPU decode path gave up: %s; decoding on the host (from %s offset %d on: %d records are counted)",
                       reason, "compressed" if isinstance(carry[1], tuple) else "byte",
                       carry[1][0] if isinstance(carry[1], tuple) else carry[1], carry[2])
    return None, carry


def _report_duplicates(options, libraries, logger):
    """--remove-duplicates: the log line, duplicates.tsv (per library: examined, duplicates, molecules, not examined because
    paired / otherwise) and duplicates_histogram.tsv (per library: molecules seen ``Copies`` times, the non-empty bins; the last
    bin is ``>=1024``) — the counts a library-complexity estimate starts from."""
    counts, hist, info = options.duplicates
    rows, bins = ["Sample\tLibrary\tExamined\tDuplicates\tMolecules\tPaired\tOther\n"], ["Sample\tLibrary\tCopies\tMolecules\n"]
    for (sample, library), (examined, dups, paired, other), h in zip(libraries, counts.tolist(), hist.tolist()):
        rows.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (sample, library, examined, dups, examined - dups, paired, other))
        bins += ["%s\t%s\t%s\t%d\n" % (sample, library, c + 1 if c + 1 < len(h) else ">=%d" % len(h), m) for c, m in enumerate(h) if m]
    (options.folder / "duplicates.tsv").write_text("".join(rows))
    (options.folder / "duplicates_histogram.tsv").write_text("".join(bins))
    examined, dups, paired, other = (int(x) for x in counts.sum(axis=0))
    logger.info("Duplicates: %d records examined, %d removed, %d molecules; not examined: %d paired, %d other",
                examined, dups, examined - dups, paired, other)
    if paired:
        logger.warning("--remove-duplicates: %d paired records were not examined (a pair's molecule needs the mate's coordinates, "
                       "which the option does not follow); they are counted as they are", paired)
    logger.debug("Duplicates: ends %s; table of %d slots, grown %d times, longest walk %d slots, mean %.3f; %d bytes of HBM",
                 options.duplicate_ends, info["slots"], info["growths"], info["longest_probe"],
                 info["probes"] / max(1, info["examined"]), info["bytes"])


def _report_depth(options, logger):
    """--depth: coverage.tsv, depth_histogram.tsv, the log line and the bedGraph of --depth-bedgraph (mapdamage_amd/depth.py)."""
    names, lengths, per_contig, hist, counts, runs, info = options.depth_result
    (options.folder / "coverage.tsv").write_text(depth_files.coverage_text(names, lengths, per_contig))
    (options.folder / "depth_histogram.tsv").write_text(depth_files.histogram_text(hist))
    if runs is not None:
        depth_files.write_bedgraph(options.depth_bedgraph, names, *runs)
    logger.info(depth_files.log_line(lengths, per_contig, counts))
    if getattr(options, "depth_regions_result", None) is not None:
        # (its four files are by_region/'s: groupings.RegionGroups.write)
        logger.info(depth_files.region_log_line(options.depth_regions_result[1]))
    logger.debug("Depth: %d intervals, %d runs of depth > 0; %d bytes of HBM", counts["intervals"], counts["runs"], info["bytes"])


def _report_pileup(options, logger):
    """--pileup-sites: pileup.tsv, pileup_summary.tsv and the log lines (mapdamage_amd/pileup.py)."""
    names, counters, refbase, call, depth, counts, info = options.pileup_result
    sites = options.pileup_sites_list
    with_call = options.pileup_call != "none"
    pileup_files.write_pileup(options.folder / "pileup.tsv", names, sites, counters, refbase, call, depth, with_call)
    values = dict(path=options.pileup_sites, min_basequal=options.pileup_min_basequal, mask_ends=options.pileup_mask_ends,
                  call=options.pileup_call, seed=options.pileup_seed, min_depth=options.pileup_min_depth,
                  single_strand=options.pileup_single_strand_mode)
    (options.folder / "pileup_summary.tsv").write_text(pileup_files.summary_text(values, counters, call, depth, counts))
    logger.info(pileup_files.log_line(values, counters, call, depth, counts))
    strangers = pileup_files.off_build(sites, refbase)
    if strangers:
        logger.warning("--pileup-sites: at %d of %d sites the reference's base is neither Ref nor Alt; the usual sign of a list "
                       "of sites made for another build of the genome", strangers, len(sites))
    logger.debug("Pileup: %d pairs of a record and a site; a list of %d pairs a round; %d bytes of HBM", counts["pairs"], info["list_pairs"], info["bytes"])
    if getattr(options, "pileup_likelihoods_result", None) is None:
        return
    # --pileup-likelihoods: the two files of the folder, the BEAGLE file and the log line
    gl, best, bases, added = options.pileup_likelihoods_result
    values["noqual_quality"] = options.pileup_noqual_quality
    t0 = time.perf_counter()
    pileup_files.write_likelihoods(options.folder / "pileup_likelihoods.tsv", names, sites, gl, best, bases)
    (options.folder / "pileup_likelihoods_summary.tsv").write_text(pileup_files.likelihoods_summary_text(values, bases, added))
    if getattr(options, "pileup_beagle", None) is not None:
        pileup_files.write_beagle(options.pileup_beagle, names, sites, gl, bases)
    logger.info(pileup_files.likelihoods_log_line(values, bases, added))
    profile = getattr(options, "pileup_damage_profile_rows", None)
    if profile is not None:
        (options.folder / "pileup_damage_profile.tsv").write_text(pileup_files.damage_profile_text(profile))
        logger.info(pileup_files.damage_profile_log_line(profile))
    logger.debug("Pileup likelihoods: the files of %d sites formatted and written in %.3f s", len(sites), time.perf_counter() - t0)


def main(argv):
    start_time = time.time()
    stages = _Stages()
    stages.mark("main")
    logging.basicConfig(format=_LOG_FORMAT, datefmt="%H:%M:%S")
    logger = logging.getLogger(__name__)
    try:
        options = parse_args(argv)
    except SystemExit as error:
        return int(error.code or 0) and 1
    import os
    if options.stats_only:
        # mapdamage/main.py:93-111: from the tables of an existing folder; one process, one GPU
        if int(os.environ.get("RANK", "0")) != 0:
            return 0
        handler = logging.FileHandler(options.folder / "Runtime_log.txt")
        handler.setFormatter(logging.Formatter(_LOG_FORMAT))
        logging.getLogger().setLevel(options.log_level)
        logging.getLogger().addHandler(handler)
        try:
            if not check_table_and_warn_if_dmg_freq_is_low(options.folder):
                logger.error("Cannot use the Bayesian estimation, terminating the program")
                return 1
            return bayesian_estimates(options, logger, device=options.device)
        finally:
            logging.getLogger().removeHandler(handler)
            handler.close()
    if options.rescale_only:
        # the rescaling pass rewrites one BAM file in file order (rescale.py:285-365): one process, one GPU — under a launcher
        # that started several ranks the others leave at once instead of waiting in a process group for rank 0's whole pass
        if int(os.environ.get("RANK", "0")) != 0:
            return 0
        options.gpus = 1
        if os.environ.get("WORLD_SIZE", "1") != "1":
            for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
                os.environ.pop(key, None)
    if options.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU: the run re-executes itself under torchrun (or is launched that way to begin with)
        import subprocess
        cmd = launch_command(list(argv), options.gpus)
        if options.print_launch:
            import json
            print(json.dumps(cmd))
            return 0
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        return subprocess.call(cmd, env=env)
    ranks = _Ranks(options)
    first = ranks.rank == 0
    # stdin, a named pipe, /dev/fd/N: opened once, here — the format sniff, the header, the device decode and a host decoder
    # that takes over all read the one Source
    options.source = None
    if is_stream(options.filename):
        from .sam import Source
        options.source = Source(options.filename)
    if options.gpu_decode and not options.rescale_only and _device_path_applies(options, ranks.world) and not os.environ.get("MDX_NO_WARM"):
        # the device's context, the decode kernels and the pinned buffer of the host's share (about a fifth of a slab's
        # inflated bytes, which are four to five times its compressed ones), beside the header, index and FASTA reads
        import threading
        try:
            pinned = _slab_bytes(options, ranks.world)
            if options.source is None or not options.source.is_stream:       # (a pipe has no size)
                pinned = min(pinned, os.path.getsize(options.filename))
        except OSError:
            pinned = 0
        options.warm_thread = threading.Thread(target=_warm_up, args=(ranks.device, pinned), daemon=True)
        options.warm_thread.start()
    # (rank 0 keeps the log file and writes the tables; the other ranks speak up only when something is wrong)
    logging.getLogger().setLevel(options.log_level if first else "WARNING")
    handler = logging.FileHandler(options.folder / "Runtime_log.txt") if first else logging.NullHandler()
    handler.setFormatter(logging.Formatter(_LOG_FORMAT))
    handler.setLevel(options.log_level)
    logging.getLogger().addHandler(handler)
    reader = None
    try:
        logger.info("Started with the command: " + " ".join(sys.argv))
        if options.rescale_only:
            logger.info("Starting rescaling...")
            return rescale_qual(options) if first else 0
        if ranks.world > 1:
            logger.info("Rank 0 of %d: one process per GPU, records sharded by slab of the file, tables summed over %s",
                        ranks.world, "RCCL" if ranks.backend == "nccl" else "gloo (host)")
        # (the host is the node's: every rank takes its share of the threads cpu.max grants, include/mdx.h mdx_host_threads)
        from .engine import load_library
        from .sam import usable_cpus
        logger.debug("Host threads of this rank: %d inflating beside the device, %d for the host decoder (LOCAL_WORLD_SIZE %s)",
                     load_library().mdx_host_threads(), usable_cpus(), os.environ.get("LOCAL_WORLD_SIZE", "1"))
        reader = BAMReader(options.filename, merge_libraries=options.merge_libraries,
                           downsample_to=options.downsample, downsample_seed=options.downsample_seed,
                           chunk_bytes=int(options.chunk_mb * (1 << 20)), source=options.source,
                           record_filter=options.record_filter,
                           sam_header_only=options.gpu_decode and _device_path_applies(options, ranks.world))
        reflengths = reader.get_references()
        if options.write_index:
            too_long = [(name, int(length)) for name, length in zip(reader.handle.header.references, reader.handle.header.lengths)
                        if int(length) > 1 << 29]
            if too_long:
                logger.error("--write-index: reference sequence %s has %d bases, and BAI cannot address a position behind 2^29 = "
                             "536870912; CSI, the index format that can, is not written", *too_long[0])
                return 1
        if not is_plain_gzip(options.ref):
            # (pysam.FastaFile indexes a file that has no index, main.py:115; a bgzip-compressed one gets .fai and .gzi)
            try:
                ensure_fasta_index(options.ref)
            except (ValueError, OSError) as error:
                logger.error("%s", error)
                return 1
        fai_lengths = read_fasta_index(str(options.ref) + ".fai")
        if not fai_lengths:
            return 1
        if not compare_sequence_dicts(fai_lengths, reflengths):
            return 1
        ref = reference_for_bam(options.ref, reader.handle.header.references)
        if getattr(ref, "path", None) is not None:
            logger.info("Reference: %s FASTA, loaded by the device (%s)", "bgzip-compressed" if is_bgzf(options.ref) else "uncompressed",
                        "BGZF blocks inflated, CRC-checked and stripped of line ends in HBM" if is_bgzf(options.ref)
                        else "stripped of line ends in HBM")
        else:
            logger.info("Reference: plain gzip FASTA, read by the host (Python reader)")
        if options.write_kept is not None and not reader.is_bam:
            logger.error("--write-kept needs BAM input: '%s' is SAM text, and writing BAM from parsed text is not part of the "
                         "option (samtools view -b in front of the run)", options.filename)
            return 1
        if options.remove_duplicates and not reader.is_bam:
            logger.error("--remove-duplicates needs BAM input: '%s' is SAM text, which the option does not take (samtools view "
                         "-b in front of the run)", options.filename)
            return 1
        if options.depth and not reader.is_bam:
            logger.error("--depth needs BAM input: '%s' is SAM text, which the option does not take (samtools view -b in front "
                         "of the run)", options.filename)
            return 1
        if options.pileup_sites is not None:
            if not reader.is_bam:
                logger.error("--pileup-sites needs BAM input: '%s' is SAM text, which the option does not take (samtools view -b "
                             "in front of the run)", options.filename)
                return 1
            try:
                options.pileup_sites_list = pileup_files.read_sites(options.pileup_sites, list(reader.handle.header.references),
                                                                    list(reader.handle.header.lengths))
            except (ValueError, OSError, UnicodeDecodeError) as error:
                logger.error("%s", error)
                return 1
            if options.pileup_single_strand_mode and options.pileup_sites_list.alleles is None:
                logger.error("--pileup-single-strand-mode needs Ref and Alt on every site: the lines of %s bring no alleles", options.pileup_sites)
                return 1
            if getattr(options, "pileup_beagle", None) is not None and options.pileup_sites_list.alleles is None:
                logger.error("--pileup-beagle needs Ref and Alt on every site: the lines of %s bring no alleles", options.pileup_sites)
                return 1
        libraries = reader.get_libraries()
        try:
            options.strata = reference_strata(options, list(reader.handle.header.references), list(reader.handle.header.lengths))
            if options.write_groups is not None:
                check_write_groups(options.write_groups, len(options.strata[0]))
        except (ValueError, OSError) as error:
            logger.error("%s", error)
            return 1
        if options.strata is not None:
            kind = groupings.kind_of(options).label
            logger.info("Tabulating %d groups of %s x %d libraries in one pass", len(options.strata[0]), kind, len(libraries))
            if len(options.strata[0]) * len(libraries) > DamageEngine.MAX_TABLES:
                logger.error("%d groups of %s x %d libraries: more than the %d tables a run can keep",
                             len(options.strata[0]), kind, len(libraries), DamageEngine.MAX_TABLES)
                return 1
        stages.mark("headers and index")

        logger.info("Reading from '%s'", options.filename)
        if options.source is None:
            logger.debug("Input: a regular file (mapped)")
        elif options.source.is_stream:
            logger.info("Input: %s from a stream (stdin, a pipe or a character device), read once as it comes in",
                        "BAM" if reader.is_bam else "SAM text")
        else:
            logger.info("Input: stdin redirected from a regular file (mapped)")
        if reader.format == SAM_BGZF:
            logger.info("Input: bgzip-compressed SAM text, %s", "inflated and parsed on the device"
                        if options.gpu_decode and _device_path_applies(options, ranks.world) else "read by the host (zlib)")
        elif reader.format == SAM_GZIP:
            logger.info("Input: plain gzip SAM text, read by the host (a gzip member has no blocks to share out among the device's lanes)")
        if options.minqual != 0:
            logger.info("Filtering out bases with a Phred score < %d", options.minqual)
        logger.info("Writing results to '%s/'", options.folder)

        try:
            tables, carry = _tabulate_on_device(options, reader, ref, libraries, logger, ranks, stages) if options.gpu_decode else (None, None)
        except (KeptTagClash, KeptIndexError) as error:
            logger.error("%s", error)
            return 1
        if tables is None and options.write_kept is not None:
            logger.error("--write-kept is written by the device decode path, which did not finish this run: nothing is "
                         "written, and the run does not go on without its output")
            return 1
        if tables is None and options.remove_duplicates:
            logger.error("--remove-duplicates marks the records on the device decode path, which did not finish this run: the "
                         "host decoder cannot go on with a set of molecules that lives on the device, and nothing is written")
            return 1
        if tables is None and options.depth:
            logger.error("--depth is gathered on the device decode path, which did not finish this run: the host decoder cannot "
                         "go on with an accumulator that lives on the device, and nothing is written")
            return 1
        if tables is None and options.pileup_sites is not None:
            logger.error("--pileup-sites is gathered on the device decode path, which did not finish this run: the host decoder "
                         "cannot go on with counters that live on the device, and nothing is written")
            return 1
        if tables is None:
            tables = _tabulate_on_host(options, reader, ref, libraries, logger, ranks, carry)
        fallbacks = getattr(options, "gpu_decode_fallbacks", 0)
        if options.gpu_decode:
            logger.log(logging.WARNING if fallbacks else logging.DEBUG, "Decode path: %s; fallbacks from the device path: %d",
                       "host decoder" if (fallbacks or not _device_path_applies(options, ranks.world)) else "device", fallbacks)
        logger.debug("Done. %d filtered alignments processed", tables.n_kept)
        logger.debug("BAM read in %f seconds", time.time() - start_time)

        if options.record_filter.active:
            _report_record_filters(options, ranks.sum_counts(options.filter_counts), logger, first)
        stages.mark("tables")
        if not first:
            return 0
        if options.strata is not None:
            # the three usual files from the sum over the groups, and the kind's directory beside them
            tables = groupings.kind_of(options).write(tables, options, options.strata, logger)
        else:
            tables.write(options.folder)
        if options.remove_duplicates:
            _report_duplicates(options, libraries, logger)
        if options.depth:
            _report_depth(options, logger)
        if options.pileup_sites is not None:
            _report_pileup(options, logger)
        if options.freq_files:
            (options.folder / "5pCtoT_freq.txt").write_text(tables.damage_frequency_text("5p", options.readplot))
            (options.folder / "3pGtoA_freq.txt").write_text(tables.damage_frequency_text("3p", options.readplot))
        usable = check_table_and_warn_if_dmg_freq_is_low(options.folder)
        if not options.no_stats:
            # main.py:241-257
            if not usable:
                logger.error("Cannot use the Bayesian estimation, terminating the program")
                return 1
            if bayesian_estimates(options, logger, ref, len(reader.handle.header.references), ranks.device):
                return 1
            stages.mark("estimates")
            if options.rescale:
                reader.close()
                reader = None
                if rescale_qual(options):
                    return 1
        logger.info("Successful run")
        logger.debug("Run completed in %f seconds", time.time() - start_time)
        stages.mark("files written")
        return 0
    except BadReadError as error:
        # the reference dies with pysam's ValueError here (align.py:33)
        logger.error("%s", error)
        raise
    except BAMError as error:
        logger.error("%s", error)
        raise
    finally:
        if reader is not None:
            reader.close()
        elif options.source is not None:
            options.source.close()
        logging.getLogger().removeHandler(handler)
        handler.close()
        ranks.close()
        stages.mark("end")
        stages.write()


def entry_point():
    """The command's exit: the tables are on disk and the log is closed when ``main`` returns, and what is left — the
    interpreter's and the HIP runtime's teardown, unpinning and unmapping a few gigabytes — is a fifth of a second the
    operating system does faster for a process that simply leaves (MDX_NO_FAST_EXIT=1: the ordinary way out)."""
    import os
    rc = main(sys.argv[1:])
    if os.environ.get("MDX_NO_FAST_EXIT"):
        return rc
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(int(rc or 0))


if __name__ == "__main__":
    sys.exit(entry_point())
