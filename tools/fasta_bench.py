"""Reference FASTA to the resident reference: a synthetic genome (3 Gb over 900 contigs by default: i.i.d. bases, an N run at
the start of every contig and in its middle, a lower-case stretch) written uncompressed and bgzip-compressed (through
sam.BgzfWriter: zlib level 6, 0xFF00-byte blocks), then the wall-clock time of ``DamageEngine.set_reference`` on

  (a) plain    the uncompressed file                       (pieces to HBM, line ends stripped there)
  (b) bgzf     the bgzipped file                           (blocks to HBM, inflated, CRC-checked and stripped there)
  (c) python   the bgzipped file through ``fasta.reference_in_memory`` + ``set_reference`` — gzip.open and a Python loop over
               every line, then one upload: what a ``*.fa.gz`` reference cost before the device took BGZF

``--repeats`` times each (the files are in the page cache from being written), and whether ``reference_fetch`` agrees between
(a) and (b) on sampled windows of every contig.  One JSON line on stdout.

    python tools/fasta_bench.py [--bases N] [--contigs K] [--repeats R] [--dir DIR] [--no-python]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_genome(bases, contigs, seed=20240108):
    """``contigs`` sequences of unequal length, ``bases`` in all: every third one half as long as its neighbours."""
    import numpy as np

    from mapdamage_amd.batch import Reference
    rng = np.random.default_rng(seed)
    weights = np.where(np.arange(contigs) % 3 == 2, 0.5, 1.0)
    sizes = np.maximum(1, (weights / weights.sum() * bases).astype(np.int64))
    letters = np.frombuffer(b"ACGT", np.uint8)
    names, seqs = [], []
    for i, size in enumerate(sizes):
        s = letters[rng.integers(0, 4, int(size), dtype=np.uint8)]
        n = int(size)
        s[:n // 50] = ord("N")                                  # a telomere's worth
        s[n // 2:n // 2 + n // 100] = ord("N")
        s[2 * n // 3:2 * n // 3 + n // 20] |= 0x20              # soft-masked
        names.append("contig%03d" % i)
        seqs.append(s.tobytes())
    return Reference(names, seqs)


def note(text):
    """Progress on stderr: the result line on stdout stays alone."""
    print("[fasta_bench] " + text, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--contigs", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", help="where the two files go (a temporary folder by default, removed afterwards)")
    ap.add_argument("--no-python", action="store_true", help="skip (c), the Python reader")
    args = ap.parse_args()
    import numpy as np

    from mapdamage_amd import fasta, sam
    from mapdamage_amd.engine import DamageEngine
    work = args.dir or tempfile.mkdtemp(prefix="mdx_fasta_bench_")
    os.makedirs(work, exist_ok=True)
    try:
        t0 = time.perf_counter()
        ref = make_genome(args.bases, args.contigs)
        names, lengths = list(ref.names), list(ref.lengths)
        plain, packed = os.path.join(work, "g.fa"), os.path.join(work, "g.fa.gz")
        fasta.write_fasta(plain, ref)
        # windows of every contig to compare, cut from the source while it is at hand
        rng = np.random.default_rng(1)
        windows = []
        for tid, n in enumerate(lengths):
            for lo in {0, max(0, n - 200)} | {int(x) for x in rng.integers(0, max(1, n - 200), 3)}:
                windows.append((tid, lo, min(n, lo + 200)))
        del ref
        t1 = time.perf_counter()
        note("genome written: %d bytes in %.1f s" % (os.path.getsize(plain), t1 - t0))
        with sam.BgzfWriter(packed) as out, open(plain, "rb") as src:
            while True:
                piece = src.read(64 << 20)
                if not piece:
                    break
                out.write(piece)
        t2 = time.perf_counter()
        note("bgzipped: %d bytes in %.1f s" % (os.path.getsize(packed), t2 - t1))
        for p in (packed + ".fai", packed + ".gzi"):
            if os.path.exists(p):
                os.remove(p)
        fasta.ensure_fasta_index(packed)          # .fai and .gzi, from the text inflated on the host: the one-time cost
        t3 = time.perf_counter()
        note(".fai and .gzi built in %.1f s" % (t3 - t2))
        result = {"tool": "fasta_bench", "bases": int(sum(lengths)), "contigs": len(names), "plain_bytes": os.path.getsize(plain),
                  "bgzf_bytes": os.path.getsize(packed), "write_plain_s": round(t1 - t0, 1), "write_bgzf_s": round(t2 - t1, 1),
                  "index_bgzf_s": round(t3 - t2, 2),
                  "fai_equal": open(packed + ".fai", "rb").read() == open(plain + ".fai", "rb").read()}
        status = 0 if result["fai_equal"] else 1
        with DamageEngine([("*", "*")], 70, 10, 0) as eng:
            def timed(make):
                t = time.perf_counter()
                eng.set_reference(make())
                eng.sync()
                return time.perf_counter() - t

            def fetch():
                return [eng.reference_fetch(tid, lo, hi) for tid, lo, hi in windows]

            runs = [("plain", lambda: fasta.reference_for_bam(plain, names)), ("bgzf", lambda: fasta.reference_for_bam(packed, names))]
            if not args.no_python:
                runs.append(("python", lambda: fasta.reference_in_memory(packed, names)))
            seen = {}
            for name, make in runs:
                times = []
                for _ in range(args.repeats):
                    times.append(timed(make))
                    note("%s: %.3f s" % (name, times[-1]))
                result["T_%s_s" % name] = [round(t, 3) for t in times]
                if name != "python":
                    result["%s_load" % name] = eng.fasta_load_stats()
                seen[name] = fetch()
            result["windows"] = len(windows)
            same = all(v == seen["plain"] for v in seen.values())
            result["fetch"] = "equal" if same else "MISMATCH"
            status = status or (0 if same else 1)
            if "python" in seen:
                result["bgzf_over_python"] = round(min(result["T_python_s"]) / max(result["T_bgzf_s"]), 1)
        print(json.dumps(result))
        return status
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
