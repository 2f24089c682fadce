"""BAM through a pipe against the same file on disk: the cli_wall workload of bench.py (config-3 records, 50 M by default, the
10 Mb genome) written as one BAM file, then three wall-clock times, each step under a time limit of its own:

  T_pipe  `cat x.bam | cat > /dev/null`                        what the pipe alone costs
  T_file  `python -m mapdamage_amd -i x.bam -r x.fa ...`        the command line on the file
  T_run   `cat x.bam | python -m mapdamage_amd -i - -r x.fa ...` the same command reading the pipe

and the stage timings of T_run (MDX_STAGE_LOG, as bench.py's cli_wall splits a run).  The aim: T_run <= max(T_pipe, T_file)
plus the run's fixed costs.  The tables of T_run must be byte-identical to those of T_file.  One JSON line on stdout.

--min-mapq Q: the file is written with MAPQ drawn from {0, 1, 24, 25, 29, 30, 37, 60, 255} (30 everywhere without), and the
command on the file is timed with and without `--min-mapq Q`, behind T_file (which has warmed the file's pages), in the order
plain, filtered, filtered, plain, ... (--repeats pairs), wall clock and the "decode and tabulate" stage of MDX_STAGE_LOG each:
`filter_runs`.  The filtered run tabulates fewer records (a third of that MAPQ set lies below 25), so what it can show is that
the filter adds no time, not what it costs per record.

    python tools/pipe_bench.py [--reads N] [--dir DIR] [--timeout S] [--min-mapq Q]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")


def timed(shell_cmd, limit, env=None):
    """``shell_cmd`` under ``timeout -k 10 limit``: (wall seconds, exit status, stderr tail)."""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), "bash", "-o", "pipefail", "-c", shell_cmd], cwd=ROOT, env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return time.perf_counter() - t0, p.returncode, p.stderr.decode(errors="replace")[-800:]


def stages(path, t_spawn, wall):
    try:
        with open(path) as fh:
            marks = json.load(fh)["stages"]
    except (OSError, ValueError, KeyError):
        return None
    stamps = [("spawn", t_spawn)] + [(k, t) for k, t in marks] + [("exit", t_spawn + wall)]
    return {stamps[i][0]: round(stamps[i][1] - stamps[i - 1][1], 4) for i in range(1, len(stamps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--dir", help="where the BAM, FASTA and outputs go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each timed step may take")
    ap.add_argument("--min-mapq", type=int, default=0, help="write varied MAPQ and time the file run with this --min-mapq as well")
    ap.add_argument("--repeats", type=int, default=3, help="pairs of runs with and without --min-mapq")
    args = ap.parse_args()
    from mapdamage_amd import fasta, sam, synth
    work = args.dir or tempfile.mkdtemp(prefix="mdx_pipe_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        ref = synth.make_genome(sizes=(("chr1", 8_000_000), ("chr2", 2_000_000), ("chrS", 500)))
        bam, fa = os.path.join(work, "x.bam"), os.path.join(work, "x.fa")
        t0 = time.perf_counter()
        # (batches of at most 25 M records, as bench.py makes the headline's: a batch's offsets into its bases are 32-bit)
        cap = 25_000_000
        batches = [synth.parallel_batch("config3_batch", ref, min(cap, args.reads - lo), seed=3000 + k, workers=16)
                   for k, lo in enumerate(range(0, args.reads, cap))]
        mapq = None
        if args.min_mapq:
            import numpy as np
            rng = np.random.default_rng(2525)
            mapq = [rng.choice(np.array([0, 1, 24, 25, 29, 30, 37, 60, 255], np.uint8), b.n) for b in batches]
        sam.write_bam(bam, batches, ref.names, ref.lengths, [{"ID": "rg1", "SM": "synthetic", "LB": "lib1"}], rg_of_record="rg1",
                      workers=16, mapq=mapq)
        fasta.write_fasta(fa, ref)
        del batches
        write_s = time.perf_counter() - t0
        cli = "%s -m mapdamage_amd -r %s --no-stats --log-level DEBUG -d " % (sys.executable, fa)
        result = {"tool": "pipe_bench", "reads": args.reads, "bam_bytes": os.path.getsize(bam), "write_bam_s": round(write_s, 1)}
        # (the file's pages warm for all three: each reads them once before)
        t_pipe, rc, err = timed("cat %s | cat > /dev/null" % bam, args.timeout)
        result["T_pipe_s"] = round(t_pipe, 3)
        if rc != 0:
            result["error"] = "T_pipe: exit %d %s" % (rc, err)
            print(json.dumps(result))
            return 1
        out_f, out_p = os.path.join(work, "file"), os.path.join(work, "pipe")
        t_file, rc, err = timed(cli + out_f + " -i " + bam, args.timeout)
        result["T_file_s"] = round(t_file, 3)
        if rc != 0:
            result["error"] = "T_file: exit %d %s" % (rc, err)
            print(json.dumps(result))
            return 1
        if args.min_mapq:
            result["min_mapq"] = args.min_mapq
            runs = {"plain": [], "filtered": []}
            order = [("plain", "filtered") if k % 2 == 0 else ("filtered", "plain") for k in range(args.repeats)]
            for k, which in enumerate(w for pair in order for w in pair):
                out_k = os.path.join(work, "%s_%d" % (which, k))
                log_k = os.path.join(work, "stages_%d.json" % k)
                extra = " --min-mapq %d" % args.min_mapq if which == "filtered" else ""
                t_spawn = time.time()
                t_k, rc, err = timed(cli + out_k + extra + " -i " + bam, args.timeout, env=dict(os.environ, MDX_STAGE_LOG=log_k))
                if rc != 0:
                    result["error"] = "%s run %d: exit %d %s" % (which, k, rc, err)
                    print(json.dumps(result))
                    return 1
                st = stages(log_k, t_spawn, t_k) or {}
                log = open(os.path.join(out_k, "Runtime_log.txt")).read()
                runs[which].append({"wall_s": round(t_k, 3), "decode_and_tabulate_s": st.get("decode and tabulate"),
                                    "device": "Decode path: device; fallbacks from the device path: 0" in log})
                if which == "filtered":
                    result["record_filters_tsv"] = open(os.path.join(out_k, "record_filters.tsv")).read()
            result["filter_runs"] = runs
        stage_log = os.path.join(work, "stages.json")
        env = dict(os.environ, MDX_STAGE_LOG=stage_log)
        t_spawn = time.time()
        t_run, rc, err = timed("cat %s | %s -i -" % (bam, cli + out_p), args.timeout, env=env)
        result["T_run_s"] = round(t_run, 3)
        if rc != 0:
            result["error"] = "T_run: exit %d %s" % (rc, err)
            print(json.dumps(result))
            return 1
        result["T_run_stages_s"] = stages(stage_log, t_spawn, t_run)
        log = open(os.path.join(out_p, "Runtime_log.txt")).read()
        result["T_run_decode_path"] = "device" if "Decode path: device; fallbacks from the device path: 0" in log else "host decoder"
        same = all(open(os.path.join(out_f, f)).read() == open(os.path.join(out_p, f)).read() for f in FILES)
        result["tables"] = "byte-identical to the file run" if same else "MISMATCH"
        result["aim_s"] = round(max(t_pipe, t_file), 3)
        print(json.dumps(result))
        return 0 if same and result["T_run_decode_path"] == "device" else 1
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
