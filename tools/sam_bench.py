"""SAM text to tables: config-3 records (10 M by default, the 10 Mb genome) written as one SAM file, then three wall-clock times
of the command line, each under a time limit of its own:

  T_file  `python -m mapdamage_amd -i x.sam -r x.fa ...`                 parsed on the device (mdx_gsam_*)
  T_pipe  `cat x.sam | python -m mapdamage_amd -i - -r x.fa ...`          the same from a pipe
  T_host  `python -m mapdamage_amd -i x.sam -r x.fa --host-decode ...`    the host parser (sam.read_sam)

with reads/s for each (records over wall time, start-up included) and whether the tables of the three are byte-identical.
--bgzf: the same records bgzipped (x.sam.gz, the project's BGZF writer) as three more legs — the file and the pipe inflated and
parsed on the device, and `--host-decode` (zlib into sam.read_sam) — with the compressed size.  One JSON line on stdout.

    python tools/sam_bench.py [--reads N] [--with-qual] [--dir DIR] [--timeout S] [--no-host] [--bgzf]"""
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
_JOB = None


def _shard_text(span):
    """SAM lines of records [lo, hi) of the workload (a forked worker: the genome is the parent's)."""
    import numpy as np

    from mapdamage_amd import layout as L
    from mapdamage_amd import synth
    ref, with_qual, k, n = _JOB[0], _JOB[1], span[0], span[1]
    b = synth.config3_batch(ref, n, seed=[3000, k], with_qual=with_qual)
    out = []
    for i in range(b.n):
        c0, c1, s0, s1 = int(b.cigar_off[i]), int(b.cigar_off[i + 1]), int(b.seq_off[i]), int(b.seq_off[i + 1])
        cig = "".join("%d%s" % (int(c) >> 4, L.CIGAR_CHARS[int(c) & 15]) for c in b.cigar[c0:c1]) or "*"
        seq = b.seq[s0:s1].tobytes().decode() or "*"
        qual = (b.qual[s0:s1] + 33).astype(np.uint8).tobytes().decode() if with_qual and s1 > s0 else "*"
        tid = int(b.tid[i])
        out.append("r%d_%d\t%d\t%s\t%d\t30\t%s\t*\t0\t%d\t%s\t%s\tRG:Z:rg1\n" % (
            k, i, int(b.flag[i]), ref.names[tid] if tid >= 0 else "*", int(b.pos[i]) + 1, cig, int(b.tlen[i]), seq, qual))
    return "".join(out).encode()


def timed(shell_cmd, limit):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), "bash", "-o", "pipefail", "-c", shell_cmd], cwd=ROOT,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return time.perf_counter() - t0, p.returncode, p.stderr.decode(errors="replace")[-800:]


def main():
    global _JOB
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--with-qual", action="store_true", help="QUAL strings (config-3 qualities) instead of '*'")
    ap.add_argument("--dir", help="where the SAM, FASTA and outputs go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds each timed step may take")
    ap.add_argument("--no-host", action="store_true", help="skip the host parser's run")
    ap.add_argument("--bgzf", action="store_true", help="the same records bgzipped: file and pipe on the device, and --host-decode")
    args = ap.parse_args()
    import multiprocessing

    from mapdamage_amd import fasta, sam, synth
    work = args.dir or tempfile.mkdtemp(prefix="mdx_sam_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        ref = synth.make_genome(sizes=(("chr1", 8_000_000), ("chr2", 2_000_000), ("chrS", 500)))
        path, fa = os.path.join(work, "x.sam"), os.path.join(work, "x.fa")
        t0 = time.perf_counter()
        _JOB = (ref, args.with_qual)
        shard = 250_000
        spans = [(k, min(shard, args.reads - lo)) for k, lo in enumerate(range(0, args.reads, shard))]
        with open(path, "wb") as out:
            out.write(sam.header_text(ref.names, ref.lengths, [{"ID": "rg1", "SM": "synthetic", "LB": "lib1"}]).encode())
            with multiprocessing.get_context("fork").Pool(16) as pool:
                for text in pool.imap(_shard_text, spans):
                    out.write(text)
        fasta.write_fasta(fa, ref)
        result = {"tool": "sam_bench", "reads": args.reads, "with_qual": args.with_qual, "sam_bytes": os.path.getsize(path),
                  "write_sam_s": round(time.perf_counter() - t0, 1)}
        cli = "%s -m mapdamage_amd -r %s --no-stats --log-level DEBUG -d " % (sys.executable, fa)
        runs = [("file", cli + os.path.join(work, "file") + " -i " + path),
                ("pipe", "cat %s | %s -i -" % (path, cli + os.path.join(work, "pipe")))]
        if not args.no_host:
            runs.append(("host", cli + os.path.join(work, "host") + " --host-decode -i " + path))
        if args.bgzf:
            gz = path + ".gz"
            t0 = time.perf_counter()
            with sam.BgzfWriter(gz) as out, open(path, "rb") as text:
                while True:
                    piece = text.read(64 << 20)
                    if not piece:
                        break
                    out.write(piece)
            result["bgzf_bytes"], result["bgzip_s"] = os.path.getsize(gz), round(time.perf_counter() - t0, 1)
            runs += [("bgzf_file", cli + os.path.join(work, "bgzf_file") + " -i " + gz),
                     ("bgzf_pipe", "cat %s | %s -i -" % (gz, cli + os.path.join(work, "bgzf_pipe")))]
            if not args.no_host:
                runs.append(("bgzf_host", cli + os.path.join(work, "bgzf_host") + " --host-decode -i " + gz))
        status = 0
        for name, cmd in runs:
            t, rc, err = timed(cmd, args.timeout)
            result["T_%s_s" % name] = round(t, 3)
            result["%s_reads_per_s" % name] = round(args.reads / t)
            if rc != 0:
                result["error"] = "%s: exit %d %s" % (name, rc, err)
                status = 1
                break
            log = open(os.path.join(work, name, "Runtime_log.txt")).read()
            if not name.endswith("host"):
                result["%s_decode_path" % name] = "device" if "Decode path: device; fallbacks from the device path: 0" in log else "host decoder"
        if status == 0:
            tables = {name: [open(os.path.join(work, name, f)).read() for f in FILES] for name, _ in runs}
            same = all(t == tables["file"] for t in tables.values())
            result["tables"] = "byte-identical" if same else "MISMATCH"
            status = 0 if same else 1
        print(json.dumps(result))
        return status
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
