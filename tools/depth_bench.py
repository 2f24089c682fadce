"""What --depth costs, in the manner of tools/write_kept_bench.py --remove-duplicates: its file — 8 M single-end 100-base
records in coordinate order with qualities on the 10 Mb genome, RATE of them drawn a second time —, then these commands timed
as cold processes, each under a time limit of its own, alternating:

  plain           `python -m mapdamage_amd -i x.bam -r x.fa --no-stats ...` on this build
  parent_plain    the same in --parent-root DIR, a built checkout of the parent commit
  depth           `--depth`
  dedup_depth     `--remove-duplicates --depth`
  depth_bedgraph  `--depth --depth-bedgraph x.bg`                    (behind the alternation: the finish's launches a second
                                                                     time, the runs to the host, the file's text)

With --targets N:WIDTH[,N:WIDTH...] a synthetic BED per entry — N targets of WIDTH bases spread evenly over the genome, one
group — and, in the same alternation, `regions_plain` (`--depth --regions`, on the parent's build too: `parent_regions_plain`)
and per BED `on_target_NxWIDTH` (`--depth --regions BED --depth-regions`); `regions_plain` uses the first BED.

Reported per command: the wall times, their median and spread (max - min); depth - plain, dedup_depth - plain and
plain - parent_plain (medians); from the log and coverage.tsv the records, the aligned and covered bases, the intervals, the
runs and the HBM the accumulator holds.  The claim to check: depth - plain is within the repeats' spread, and so is
plain - parent_plain.  One JSON line on stdout.

    python tools/depth_bench.py [--reads N] [--repeats K] [--duplicate-rate RATE] [--dir DIR] [--timeout S] [--parent-root DIR]
                                [--targets N:WIDTH[,N:WIDTH...]]"""
import argparse
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.write_kept_bench import FILES, timed     # noqa: E402


def write_targets(path, ref, n, width):
    """``n`` targets of ``width`` bases, spread evenly over the sequences in proportion to their lengths (rounded down), apart from each other."""
    total = sum(int(x) for x in ref.lengths)
    with open(path, "w") as out:
        for name, length in zip(ref.names, ref.lengths):
            share = n * int(length) // total
            if share == 0:          # (a sequence too short for a target of its own gets none)
                continue
            step = int(length) // share
            if step <= width:
                raise SystemExit("--targets %d:%d: the targets of %s would touch" % (n, width, name))
            for k in range(share):
                out.write("%s\t%d\t%d\n" % (name, k * step, k * step + width))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--duplicate-rate", type=float, default=0.3)
    ap.add_argument("--dir", help="where the BAM, FASTA and outputs go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each timed command may take")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit: `plain` is timed there as well")
    ap.add_argument("--targets", help="N:WIDTH[,N:WIDTH...]: a synthetic BED of N targets of WIDTH bases each; times --depth-regions with every one")
    args = ap.parse_args()
    import numpy as np

    from mapdamage_amd import fasta, sam, synth
    work = args.dir or tempfile.mkdtemp(prefix="mdx_depth_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        ref = synth.make_genome()
        bam, fa = os.path.join(work, "x.bam"), os.path.join(work, "x.fa")
        t0 = time.perf_counter()
        n_dup = int(round(args.reads * args.duplicate_rate))
        batch = synth.make_reads(ref, args.reads - n_dup, args.seed, read_len=100, paired=False, frac_softclip=0.10, frac_ins=0.04, frac_del=0.04,
                                 frac_skip=0.002, frac_hardclip=0.001, contigs=[0, 1], with_qual=True, sort=True)
        pick = np.sort(np.concatenate([np.arange(batch.n), np.random.default_rng(args.seed).integers(0, batch.n, n_dup)]), kind="stable")
        batch = batch.take(pick)
        sam.write_bam(bam, batch, ref.names, ref.lengths, [{"ID": "rg1", "SM": "synthetic", "LB": "lib1"}], rg_of_record=["rg1"] * args.reads)
        fasta.write_fasta(fa, ref)
        n_counted = int(((batch.flag & 0xF04) == 0).sum())
        del batch
        result = {"tool": "depth_bench", "reads": args.reads, "counted": n_counted, "reference_bases": int(sum(ref.lengths)),
                  "bam_bytes": os.path.getsize(bam), "write_bam_s": round(time.perf_counter() - t0, 1), "repeats": args.repeats,
                  "sorted": True, "duplicate_rate": args.duplicate_rate}
        base = [sys.executable, "-m", "mapdamage_amd", "-i", bam, "-r", fa, "--no-stats", "--log-level", "DEBUG"]
        legs = [("plain", ROOT, [])]
        if args.parent_root:
            legs.append(("parent_plain", os.path.abspath(args.parent_root), []))
        legs += [("depth", ROOT, ["--depth"]), ("dedup_depth", ROOT, ["--remove-duplicates", "--depth"])]
        beds = []
        for entry in (args.targets.split(",") if args.targets else []):
            n, width = (int(x) for x in entry.split(":"))
            beds.append(("%dx%d" % (n, width), write_targets(os.path.join(work, "targets_%dx%d.bed" % (n, width)), ref, n, width)))
        if beds:
            legs.append(("regions_plain", ROOT, ["--depth", "--regions", beds[0][1]]))
            if args.parent_root:
                legs.append(("parent_regions_plain", os.path.abspath(args.parent_root), ["--depth", "--regions", beds[0][1]]))
            legs += [("on_target_" + name, ROOT, ["--depth", "--regions", bed, "--depth-regions"]) for name, bed in beds]
        # (behind the alternation, on its own: a leg that writes a file of its size would sit in front of `plain` in every round)
        bedgraph = ("depth_bedgraph", ROOT, ["--depth", "--depth-bedgraph", os.path.join(work, "x.bg")])
        times = {name: [] for name, _, _ in legs + [bedgraph]}
        status = 0
        for round_legs in [legs] * args.repeats + [[bedgraph]] * args.repeats:
            for name, root, extra in round_legs:
                t, rc, err = timed(base + ["-d", os.path.join(work, name)] + extra, args.timeout, root)
                if rc != 0:
                    result["error"] = "%s: exit %d %s" % (name, rc, err)
                    status = 1
                    break
                times[name].append(round(t, 3))
            if status:
                break
        legs.append(bedgraph)
        for name, _, _ in legs:
            ts = times[name]
            if not ts:
                continue
            med = statistics.median(ts)
            result[name] = {"wall_s": ts, "median_s": round(med, 3), "spread_s": round(max(ts) - min(ts), 3), "reads_per_s": round(args.reads / med)}
            log = open(os.path.join(work, name, "Runtime_log.txt")).read()
            result[name]["decode_path"] = "device" if "Decode path: device; fallbacks from the device path: 0" in log else "host decoder"
            coverage = os.path.join(work, name, "coverage.tsv")
            if os.path.exists(coverage):
                star = open(coverage).read().splitlines()[-1].split("\t")
                result[name].update(records=int(star[2]), covered=int(star[3]), breadth=float(star[4]), aligned_bases=int(star[5]),
                                    mean_depth=float(star[6]), max_depth=int(star[7]))
                m = re.search(r"Depth: (\d+) intervals, (\d+) runs of depth > 0; (\d+) bytes of HBM", log)
                if m:
                    result[name].update(intervals=int(m.group(1)), runs=int(m.group(2)), hbm_bytes=int(m.group(3)))
        if status == 0:
            for name in ("depth", "dedup_depth", "depth_bedgraph"):
                result["%s_minus_plain_s" % name] = round(result[name]["median_s"] - result["plain"]["median_s"], 3)
            for name, bed in beds:
                leg = result["on_target_" + name]
                leg["minus_regions_plain_s"] = round(leg["median_s"] - result["regions_plain"]["median_s"], 3)
                leg["targets"] = sum(1 for _ in open(bed))
                leg["regions_depth_bytes"] = os.path.getsize(os.path.join(work, "on_target_" + name, "by_region", "regions_depth.tsv"))
                leg["log_line"] = re.search(r"Depth on target: .*", open(os.path.join(work, "on_target_" + name, "Runtime_log.txt")).read()).group(0)
            if beds and args.parent_root:
                result["regions_plain_minus_parent_regions_plain_s"] = round(result["regions_plain"]["median_s"] - result["parent_regions_plain"]["median_s"], 3)
            if args.parent_root:
                result["plain_minus_parent_plain_s"] = round(result["plain"]["median_s"] - result["parent_plain"]["median_s"], 3)
                result["depth_minus_parent_plain_s"] = round(result["depth"]["median_s"] - result["parent_plain"]["median_s"], 3)
            result["depth_bedgraph"]["bedgraph_bytes"] = os.path.getsize(os.path.join(work, "x.bg"))
            tables = {name: [open(os.path.join(work, name, f)).read() for f in FILES] for name, _, _ in legs}
            # (the leg that drops the duplicates counts other records; the others agree with `plain`, the parent's too)
            same = all(t == tables["plain"] for name, t in tables.items() if name != "dedup_depth")
            result["usual_tables"] = "byte-identical" if same else "MISMATCH"
            outside = int(re.search(r"; (\d+) records outside their sequence", open(os.path.join(work, "depth", "Runtime_log.txt")).read()).group(1))
            result["depth"]["outside"] = outside
            if result["depth"]["records"] + outside != n_counted:
                result["error"] = "coverage.tsv counts %d records and %d outside, the file holds %d the flag filter keeps" % (
                    result["depth"]["records"], outside, n_counted)
            status = 0 if same and "error" not in result else 1
        print(json.dumps(result))
        return status
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
