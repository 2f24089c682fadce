"""What --pileup-sites costs, in the manner of tools/depth_bench.py: its file — 8 M single-end 100-base records in coordinate
order with qualities on the 10 Mb genome, RATE of them drawn a second time —, two lists of sites, then these commands timed as
cold processes, each under a time limit of its own, alternating:

  plain           `python -m mapdamage_amd -i x.bam -r x.fa --no-stats ...` on this build
  parent_plain    the same in --parent-root DIR, a built checkout of the parent commit
  sparse          `--pileup-sites sparse.txt`: one site per 2 500 bases, with alleles (a SNP panel's density)
  dense           `--pileup-sites dense.txt`: every base of the first 100 kb (a capture's density)
  sparse_masked   `--pileup-sites sparse.txt --pileup-min-basequal 20 --pileup-mask-ends 2,2`: the stream brings its qualities
  write_kept      `--write-kept x.kept.bam`: the first half of the route the option replaces (the genotyper that inflates the
                  file again is not timed)
with --likelihoods these instead of the last two:
  sparse_gl       `--pileup-sites sparse.txt --pileup-likelihoods`
  dense_gl        `--pileup-sites dense.txt --pileup-likelihoods`
and then per list the difference to the same list without the option, and from the log the seconds the host took to format and
write the likelihood files.
With --damage-profile [FILE] only plain, parent_plain, sparse_gl, dense_gl and
  sparse_gld      `--pileup-sites sparse.txt --pileup-likelihoods --pileup-damage-profile FILE`
  dense_gld       `--pileup-sites dense.txt --pileup-likelihoods --pileup-damage-profile FILE`
FILE by default the misincorporation.txt that `plain` has just written (the two-run workflow); and per list the difference to
the same list under --pileup-likelihoods alone.

Reported per command: the wall times, their median and spread (max - min); the medians' differences from `plain`, and
plain - parent_plain; from the log the option's line.  The claim to check: plain - parent_plain is within the repeats' spread
(nothing new runs when the option is off).  One JSON line on stdout.

    python tools/pileup_bench.py [--reads N] [--repeats K] [--duplicate-rate RATE] [--dir DIR] [--timeout S] [--parent-root DIR] [--likelihoods]
                                  [--damage-profile [FILE]]"""
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

SPARSE_STEP = 2500
DENSE_BASES = 100_000


def write_sites(work, ref):
    """sparse.txt: a site every SPARSE_STEP bases of every sequence, the reference's letter and the next one as alleles;
    dense.txt: every base of the first DENSE_BASES of the first sequence, without alleles.  -> (paths, numbers of sites)"""
    sparse, dense = os.path.join(work, "sparse.txt"), os.path.join(work, "dense.txt")
    n_sparse = 0
    with open(sparse, "w") as out:
        for name, length, seq in zip(ref.names, ref.lengths, ref.seqs):
            for p in range(SPARSE_STEP // 2, int(length), SPARSE_STEP):
                letter = chr(seq[p]).upper()
                letter = letter if letter in "ACGT" else "A"
                out.write("%s\t%d\t%s\t%s\n" % (name, p + 1, letter, "ACGT"[("ACGT".index(letter) + 1) % 4]))
                n_sparse += 1
    n_dense = min(DENSE_BASES, int(ref.lengths[0]))
    with open(dense, "w") as out:
        out.write("".join("%s\t%d\n" % (ref.names[0], p + 1) for p in range(n_dense)))
    return (sparse, dense), (n_sparse, n_dense)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--duplicate-rate", type=float, default=0.3)
    ap.add_argument("--dir", help="where the BAM, FASTA and outputs go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each timed command may take")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit: `plain` is timed there as well")
    ap.add_argument("--likelihoods", action="store_true", help="time --pileup-likelihoods on either list instead of sparse_masked and write_kept")
    ap.add_argument("--damage-profile", nargs="?", const="", default=None, metavar="FILE",
                    help="time --pileup-likelihoods with and without --pileup-damage-profile FILE on either list (FILE: by default plain's misincorporation.txt)")
    args = ap.parse_args()
    import numpy as np

    from mapdamage_amd import fasta, sam, synth
    work = args.dir or tempfile.mkdtemp(prefix="mdx_pileup_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        ref = synth.make_genome()
        bam, fa = os.path.join(work, "x.bam"), os.path.join(work, "x.fa")
        t0 = time.perf_counter()
        if not (os.path.exists(bam) and os.path.exists(fa)):        # (a --dir that holds the file of an earlier run: not written again)
            n_dup = int(round(args.reads * args.duplicate_rate))
            batch = synth.make_reads(ref, args.reads - n_dup, args.seed, read_len=100, paired=False, frac_softclip=0.10, frac_ins=0.04, frac_del=0.04,
                                     frac_skip=0.002, frac_hardclip=0.001, contigs=[0, 1], with_qual=True, sort=True)
            pick = np.sort(np.concatenate([np.arange(batch.n), np.random.default_rng(args.seed).integers(0, batch.n, n_dup)]), kind="stable")
            batch = batch.take(pick)
            sam.write_bam(bam, batch, ref.names, ref.lengths, [{"ID": "rg1", "SM": "synthetic", "LB": "lib1"}], rg_of_record=["rg1"] * args.reads)
            fasta.write_fasta(fa, ref)
            del batch
        (sparse, dense), (n_sparse, n_dense) = write_sites(work, ref)
        result = {"tool": "pileup_bench", "reads": args.reads, "reference_bases": int(sum(ref.lengths)), "bam_bytes": os.path.getsize(bam),
                  "write_bam_s": round(time.perf_counter() - t0, 1), "repeats": args.repeats, "sorted": True, "duplicate_rate": args.duplicate_rate,
                  "sparse_sites": n_sparse, "dense_sites": n_dense}
        base = [sys.executable, "-m", "mapdamage_amd", "-i", bam, "-r", fa, "--no-stats", "--log-level", "DEBUG"]
        legs = [("plain", ROOT, [])]
        if args.parent_root:
            legs.append(("parent_plain", os.path.abspath(args.parent_root), []))
        if args.damage_profile is not None:
            profile = args.damage_profile or os.path.join(work, "plain", "misincorporation.txt")
            for name, sites in (("sparse", sparse), ("dense", dense)):
                legs += [(name + "_gl", ROOT, ["--pileup-sites", sites, "--pileup-likelihoods"]),
                         (name + "_gld", ROOT, ["--pileup-sites", sites, "--pileup-likelihoods", "--pileup-damage-profile", profile])]
        else:
            legs += [("sparse", ROOT, ["--pileup-sites", sparse]), ("dense", ROOT, ["--pileup-sites", dense])]
        if args.damage_profile is not None:
            pass
        elif args.likelihoods:
            legs += [("sparse_gl", ROOT, ["--pileup-sites", sparse, "--pileup-likelihoods"]), ("dense_gl", ROOT, ["--pileup-sites", dense, "--pileup-likelihoods"])]
        else:
            legs += [("sparse_masked", ROOT, ["--pileup-sites", sparse, "--pileup-min-basequal", "20", "--pileup-mask-ends", "2,2"]),
                     ("write_kept", ROOT, ["--write-kept", os.path.join(work, "x.kept.bam")])]
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
            line = re.search(r"Pileup: \d+ sites.*", log)
            if line:
                result[name]["log_line"] = line.group(0)
                m = re.search(r"Pileup: (\d+) pairs of a record and a site; a list of (\d+) pairs a round; (\d+) bytes of HBM", log)
                result[name].update(pairs=int(m.group(1)), list_pairs=int(m.group(2)), hbm_bytes=int(m.group(3)),
                                    pileup_tsv_bytes=os.path.getsize(os.path.join(work, name, "pileup.tsv")))
            line = re.search(r"Pileup likelihoods: \d+ sites, .*", log)
            if line:
                m = re.search(r"Pileup likelihoods: the files of \d+ sites formatted and written in ([0-9.]+) s", log)
                result[name].update(likelihoods_log_line=line.group(0), likelihoods_format_s=float(m.group(1)),
                                    likelihoods_tsv_bytes=os.path.getsize(os.path.join(work, name, "pileup_likelihoods.tsv")))
            line = re.search(r"Pileup damage profile: .*", log)
            if line:
                result[name]["damage_profile_log_line"] = line.group(0)
        if status == 0:
            for name, _, _ in legs:
                if name not in ("plain", "parent_plain"):
                    result["%s_minus_plain_s" % name] = round(result[name]["median_s"] - result["plain"]["median_s"], 3)
            if args.damage_profile is not None:
                for name in ("sparse", "dense"):
                    result["%s_gld_minus_%s_gl_s" % (name, name)] = round(result[name + "_gld"]["median_s"] - result[name + "_gl"]["median_s"], 3)
            elif args.likelihoods:
                for name in ("sparse", "dense"):
                    result["%s_gl_minus_%s_s" % (name, name)] = round(result[name + "_gl"]["median_s"] - result[name]["median_s"], 3)
            if args.parent_root:
                result["plain_minus_parent_plain_s"] = round(result["plain"]["median_s"] - result["parent_plain"]["median_s"], 3)
            tables = {name: [open(os.path.join(work, name, f)).read() for f in FILES] for name, _, _ in legs}
            same = all(t == tables["plain"] for t in tables.values())
            result["usual_tables"] = "byte-identical" if same else "MISMATCH"
            status = 0 if same else 1
        print(json.dumps(result))
        return status
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
