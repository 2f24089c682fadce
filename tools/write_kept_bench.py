"""What --write-kept costs: config-3 records with qualities (8 M by default, the 10 Mb genome, qualities from a seed) written as
one BAM, then three commands timed as cold processes, each under a time limit of its own:

  plain   `python -m mapdamage_amd -i x.bam -r x.fa --no-stats ...`                                       what a run did before
  kept    the same with `--write-kept kept.bam`                                                          every counted record
  pmd     the same with `--by-pmd-score --pmd-thresholds 3 --write-kept pmd.bam --write-groups 1`        the top PMD group
  --tags adds two more:
  pmd_all     `--by-pmd-score --pmd-thresholds 3 --write-kept pmd_all.bam`                               every counted record
  pmd_tagged  the same with `--tag-group XG --tag-pmd-score DS`                                          ... with its two tags
  --index instead: the records in coordinate order (synth's sort=True), and the legs
  plain, kept as above, and
  kept_index  `--write-kept kept_index.bam --write-index`                                                ... and its BAI index
  --mask-ends K5[,K3] instead: the legs plain, kept, and one per --mask-what,
  mask_all, mask_transitions, mask_mismatches  `--write-kept mask_X.bam --mask-ends K5,K3 --mask-what X`   ... handed on masked
  --calmd instead: the legs plain, kept, and
  calmd       `--write-kept calmd.bam --calmd`                                                           ... NM and MD recomputed
  mask_calmd  `--write-kept mask_calmd.bam --mask-ends 2,2 --calmd`                                      ... behind the mask
  --remove-duplicates RATE instead: single-end records in coordinate order (its paired ones would all go unexamined), RATE of
  them later copies of another record, and the legs plain, kept, and
  dedup       `--remove-duplicates`                                                                      the later copies marked
  dedup_kept  `--remove-duplicates --write-kept dedup_kept.bam`                                          ... and the rest written

The repeats alternate the commands (plain, kept, pmd, plain, ...), three of each by default.  Reported per command: the wall
times, their median and spread (max - min), reads/s from the median, and for the two writers the records and bytes written
(write_kept.tsv) and the file's size.  kept - plain and pmd - plain (medians) are the feature's cost, pmd_tagged - pmd_all that
of the tags (12 bytes a record, the score column, the walk over every written record's tags), kept_index - kept that of the
index (four launches and two small copies per slab, the file's assembly on the host), mask_X - kept that of the mask (one
launch per slab, in place in the stream; mask_ends.tsv gives the records and bases it masked), calmd - kept that of the
recomputed tags (five launches and sixteen bytes back per slab, a second stream; calmd.tsv gives the records recomputed and
skipped), dedup - plain and dedup_kept - kept that of the duplicate stage (six small launches per slab; the table's slots, its
growths, the longest and the mean walk of an insert and the HBM it holds are taken from the log, the counts from
duplicates.tsv).  --parent-root DIR: a built checkout of the parent commit; `plain` is then also timed there — with --calmd `kept` as
well —, in the same alternation: a difference between the two beyond the spread means the option-less path has changed.
One JSON line on stdout.

    python tools/write_kept_bench.py [--reads N] [--repeats K] [--dir DIR] [--timeout S] [--parent-root DIR] [--tags | --index | --mask-ends K | --calmd | --remove-duplicates RATE]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")


def timed(argv, limit, root):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=root, env=dict(os.environ, PYTHONPATH=root),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return time.perf_counter() - t0, p.returncode, p.stderr.decode(errors="replace")[-800:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--dir", help="where the BAM, FASTA and outputs go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each timed command may take")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit: `plain` is timed there as well")
    ap.add_argument("--tags", action="store_true", help="also time --by-pmd-score --write-kept with and without --tag-group / --tag-pmd-score")
    ap.add_argument("--index", action="store_true", help="coordinate-sorted records; time --write-kept with and without --write-index")
    ap.add_argument("--mask-ends", metavar="K5[,K3]", help="time --write-kept with and without --mask-ends K5[,K3], for each --mask-what")
    ap.add_argument("--calmd", action="store_true", help="time --write-kept with and without --calmd, and with --mask-ends 2,2 --calmd")
    ap.add_argument("--remove-duplicates", type=float, metavar="RATE", help="single-end sorted records, RATE of them later copies; time "
                    "--remove-duplicates with and without --write-kept")
    args = ap.parse_args()
    import numpy as np

    from mapdamage_amd import fasta, sam, synth
    work = args.dir or tempfile.mkdtemp(prefix="mdx_write_kept_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        ref = synth.make_genome()
        bam, fa = os.path.join(work, "x.bam"), os.path.join(work, "x.fa")
        t0 = time.perf_counter()
        if args.remove_duplicates is not None:
            # (config-3's records, single-end, in coordinate order; the copies are whole records drawn again, each behind its first)
            n_dup = int(round(args.reads * args.remove_duplicates))
            batch = synth.make_reads(ref, args.reads - n_dup, args.seed, read_len=100, paired=False, frac_softclip=0.10, frac_ins=0.04, frac_del=0.04,
                                     frac_skip=0.002, frac_hardclip=0.001, contigs=[0, 1], with_qual=True, sort=True)
            pick = np.sort(np.concatenate([np.arange(batch.n), np.random.default_rng(args.seed).integers(0, batch.n, n_dup)]), kind="stable")
            batch = batch.take(pick)
        elif args.index:
            # (config-3's records — synth.config3_batch — in coordinate order)
            batch = synth.make_reads(ref, args.reads, args.seed, read_len=100, paired=True, frac_softclip=0.10, frac_ins=0.04, frac_del=0.04,
                                     frac_skip=0.002, frac_hardclip=0.001, contigs=[0, 1], with_qual=True, sort=True)
        else:
            batch = synth.config3_batch(ref, args.reads, seed=args.seed, with_qual=True)
        sam.write_bam(bam, batch, ref.names, ref.lengths, [{"ID": "rg1", "SM": "synthetic", "LB": "lib1"}],
                      rg_of_record=["rg1"] * args.reads)
        fasta.write_fasta(fa, ref)
        n_counted = int(((batch.flag & 0xF04) == 0).sum())
        del batch
        result = {"tool": "write_kept_bench", "reads": args.reads, "counted": n_counted, "bam_bytes": os.path.getsize(bam),
                  "write_bam_s": round(time.perf_counter() - t0, 1), "repeats": args.repeats}
        base = [sys.executable, "-m", "mapdamage_amd", "-i", bam, "-r", fa, "--no-stats", "--log-level", "DEBUG"]
        legs = [("plain", ROOT, []), ("kept", ROOT, ["--write-kept", os.path.join(work, "kept.bam")]),
                ("pmd", ROOT, ["--by-pmd-score", "--pmd-thresholds", "3", "--write-kept", os.path.join(work, "pmd.bam"), "--write-groups", "1"])]
        if args.index:
            legs = legs[:2] + [("kept_index", ROOT, ["--write-kept", os.path.join(work, "kept_index.bam"), "--write-index"])]
            result["sorted"] = True
        if args.mask_ends:
            legs = legs[:2] + [("mask_" + what, ROOT, ["--write-kept", os.path.join(work, "mask_%s.bam" % what), "--mask-ends", args.mask_ends,
                                                       "--mask-what", what]) for what in ("all", "transitions", "mismatches")]
        if args.calmd:
            legs = legs[:2] + [("calmd", ROOT, ["--write-kept", os.path.join(work, "calmd.bam"), "--calmd"]),
                               ("mask_calmd", ROOT, ["--write-kept", os.path.join(work, "mask_calmd.bam"), "--mask-ends", "2,2", "--calmd"])]
        if args.remove_duplicates is not None:
            legs = legs[:2] + [("dedup", ROOT, ["--remove-duplicates"]),
                               ("dedup_kept", ROOT, ["--remove-duplicates", "--write-kept", os.path.join(work, "dedup_kept.bam")])]
            result["sorted"], result["duplicate_rate"] = True, args.remove_duplicates
        if args.tags:
            pmd_all = ["--by-pmd-score", "--pmd-thresholds", "3", "--write-kept"]
            legs += [("pmd_all", ROOT, pmd_all + [os.path.join(work, "pmd_all.bam")]),
                     ("pmd_tagged", ROOT, pmd_all + [os.path.join(work, "pmd_tagged.bam"), "--tag-group", "XG", "--tag-pmd-score", "DS"])]
        if args.parent_root:
            legs.insert(1, ("parent_plain", os.path.abspath(args.parent_root), []))
            if args.calmd:
                legs.insert(3, ("parent_kept", os.path.abspath(args.parent_root), ["--write-kept", os.path.join(work, "parent_kept.bam")]))
        times = {name: [] for name, _, _ in legs}
        status = 0
        for _ in range(args.repeats):
            for name, root, extra in legs:
                t, rc, err = timed(base + ["-d", os.path.join(work, name)] + extra, args.timeout, root)
                if rc != 0:
                    result["error"] = "%s: exit %d %s" % (name, rc, err)
                    status = 1
                    break
                times[name].append(round(t, 3))
            if status:
                break
        for name, _, _ in legs:
            ts = times[name]
            if not ts:
                continue
            med = statistics.median(ts)
            result[name] = {"wall_s": ts, "median_s": round(med, 3), "spread_s": round(max(ts) - min(ts), 3), "reads_per_s": round(args.reads / med)}
            log = open(os.path.join(work, name, "Runtime_log.txt")).read()
            result[name]["decode_path"] = "device" if "Decode path: device; fallbacks from the device path: 0" in log else "host decoder"
            tsv = os.path.join(work, name, "write_kept.tsv")
            if os.path.exists(tsv):
                path, groups, records, raw = open(tsv).read().splitlines()[1].split("\t")
                result[name].update(groups=groups, records_written=int(records), uncompressed_bytes=int(raw), file_bytes=os.path.getsize(path))
        if status == 0:
            for name in ("kept",) if args.index or args.mask_ends or args.calmd or args.remove_duplicates is not None else ("kept", "pmd"):
                result["%s_minus_plain_s" % name] = round(result[name]["median_s"] - result["plain"]["median_s"], 3)
            if args.index:
                result["kept_index_minus_kept_s"] = round(result["kept_index"]["median_s"] - result["kept"]["median_s"], 3)
                bai = os.path.join(work, "kept_index.bam.bai")
                result["kept_index"]["index_bytes"] = os.path.getsize(bai) if os.path.exists(bai) else None
                line = [ln for ln in open(os.path.join(work, "kept_index", "Runtime_log.txt")).read().splitlines() if "Wrote index" in ln]
                result["kept_index"]["log"] = line[-1].split(" (", 1)[1].rstrip(")") if line else None
                same_file = open(os.path.join(work, "kept.bam"), "rb").read() == open(os.path.join(work, "kept_index.bam"), "rb").read()
                if not same_file or result["kept_index"]["index_bytes"] is None:
                    result["error"] = "kept_index.bam differs from kept.bam, or no index was written"
            if args.mask_ends:
                for what in ("all", "transitions", "mismatches"):
                    leg = result["mask_" + what]
                    result["mask_%s_minus_kept_s" % what] = round(leg["median_s"] - result["kept"]["median_s"], 3)
                    row = open(os.path.join(work, "mask_" + what, "mask_ends.tsv")).read().splitlines()[1].split("\t")
                    leg.update(masked_records=int(row[5]), masked_bases=int(row[6]))
                    if (leg["records_written"], leg["uncompressed_bytes"]) != (result["kept"]["records_written"], result["kept"]["uncompressed_bytes"]):
                        result["error"] = "mask_%s.bam does not hold kept.bam's records and bytes" % what
            if args.calmd:
                for name in ("calmd", "mask_calmd"):
                    leg = result[name]
                    result["%s_minus_kept_s" % name] = round(leg["median_s"] - result["kept"]["median_s"], 3)
                    row = open(os.path.join(work, name, "calmd.tsv")).read().splitlines()[1].split("\t")
                    leg.update(recomputed=int(row[2]), skipped=int(row[3]), had_tags=int(row[4]))
                    if leg["records_written"] != result["kept"]["records_written"] or leg["recomputed"] + leg["skipped"] != leg["records_written"]:
                        result["error"] = "%s.bam does not hold kept.bam's records, or calmd.tsv does not add up" % name
                if args.parent_root:
                    result["kept_minus_parent_kept_s"] = round(result["kept"]["median_s"] - result["parent_kept"]["median_s"], 3)
                    if open(os.path.join(work, "kept.bam"), "rb").read() != open(os.path.join(work, "parent_kept.bam"), "rb").read():
                        result["error"] = "kept.bam differs from the parent's"
            if args.remove_duplicates is not None:
                import re
                result["dedup_minus_plain_s"] = round(result["dedup"]["median_s"] - result["plain"]["median_s"], 3)
                result["dedup_kept_minus_kept_s"] = round(result["dedup_kept"]["median_s"] - result["kept"]["median_s"], 3)
                for name in ("dedup", "dedup_kept"):
                    row = [int(x) for x in open(os.path.join(work, name, "duplicates.tsv")).read().splitlines()[1].split("\t")[2:]]
                    result[name].update(zip(("examined", "duplicates", "molecules", "paired", "other"), row))
                    log = open(os.path.join(work, name, "Runtime_log.txt")).read()
                    m = re.search(r"table of (\d+) slots, grown (\d+) times, longest walk (\d+) slots, mean ([0-9.]+); (\d+) bytes of HBM", log)
                    if m:
                        result[name].update(slots=int(m.group(1)), growths=int(m.group(2)), longest_probe=int(m.group(3)), mean_probe=float(m.group(4)),
                                            hbm_bytes=int(m.group(5)), hbm_bytes_per_examined=round(int(m.group(5)) / max(1, row[0]), 1))
                if result["dedup_kept"]["records_written"] != n_counted - result["dedup_kept"]["duplicates"]:
                    result["error"] = "dedup_kept.bam: %d records, %d counted without the option, %d duplicates" % (
                        result["dedup_kept"]["records_written"], n_counted, result["dedup_kept"]["duplicates"])
            if args.tags:
                result["pmd_tagged_minus_pmd_all_s"] = round(result["pmd_tagged"]["median_s"] - result["pmd_all"]["median_s"], 3)
                extra = result["pmd_tagged"]["uncompressed_bytes"] - result["pmd_all"]["uncompressed_bytes"]
                if result["pmd_tagged"]["records_written"] != n_counted or extra != 12 * n_counted:
                    result["error"] = "pmd_tagged.bam: %d records, %d bytes more than pmd_all.bam; %d records counted" % (
                        result["pmd_tagged"]["records_written"], extra, n_counted)
            tables = {name: [open(os.path.join(work, name, f)).read() for f in FILES] for name, _, _ in legs}
            # (the legs that drop the duplicates agree among themselves, the others with `plain`)
            same = all(t == tables["dedup" if name.startswith("dedup") else "plain"] for name, t in tables.items())
            result["usual_tables"] = "byte-identical" if same else "MISMATCH"
            if result["kept"]["records_written"] != n_counted:
                result["error"] = "kept.bam holds %d records, the run counted %d" % (result["kept"]["records_written"], n_counted)
            status = 0 if same and "error" not in result else 1
        print(json.dumps(result))
        return status
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
