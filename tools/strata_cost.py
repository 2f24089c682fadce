"""What the strata key costs (include/mdx.h mdx_set_strata): 16 M config-3 records over a genome of 8 contigs, tabulated
(a) by a stratified context of 1 library x 8 groups — the key column made on the device in front of the launch — and
(b) by a plain context of 8 libraries whose lib column was set to the same key on the host: what the library could do
before it had strata, the baseline.  Both over a resident 4-bit batch WITHOUT its bucketed copy (mdx_batch::libsort), as
the views of the file decoders come: the sort by key runs inside every call, in (a) behind the key kernel.  The two are run
interleaved in one process — a, b, a, b, ... — and timed on the wall clock, a call and its synchronisation, so that whatever
the box does to one it does to the other; the spread of (b)'s own repeats is quoted beside the ratio.  The key moves 10
bytes per record (flag, tid and lib in, a key out) against the 240 of the tabulation: a ratio near 1.03 is what the
arithmetic allows.  The two blocks are compared bit for bit on the way.  Run on the GPU box:
    python tools/strata_cost.py [--out FILE] [--regions] [records] [repeats]
--regions: (a) is a region-stratified context (mdx_set_strata_regions) of 1 library x 8 groups — 4 000 regions of 150 bases
per contig in seven groups and the rest, so the binary search of a sequence's slice takes 12 steps — and (b)'s lib column
holds the same key made on the host with numpy.  The region key reads pos, the two CIGAR offsets and the CIGAR words (one
to three for most records) on top of the 10 bytes of the tid key: some 26 bytes per record, and the search's loads, which
stay in the L2 (384 KB of intervals).  No bound is fixed: the rows say what was seen."""
import ctypes
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mapdamage_amd import synth  # noqa: E402
from mapdamage_amd.engine import DamageEngine  # noqa: E402

N_CONTIG = 8
CONFIG3 = dict(read_len=100, paired=True, frac_softclip=0.10, frac_ins=0.04, frac_del=0.04, frac_skip=0.002, frac_hardclip=0.001,
               contigs=list(range(N_CONTIG)))


def resident_without_sort(eng, batch):
    """The batch in HBM and a view of it that does not bring the bucketed copy."""
    db = eng.upload(batch, packed=True)
    view = type(db.dev)()
    ctypes.memmove(ctypes.byref(view), ctypes.byref(db.dev), ctypes.sizeof(view))
    view.libsort = None
    return db, view


def one_call(eng, view):
    t0 = time.perf_counter()
    eng.tabulate_view(view)
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


REGIONS_PER_CONTIG, REGION_BASES, REGION_STRIDE = 4000, 150, 312


def region_columns():
    """(iv_off, iv_start, iv_end, iv_group): on every contig 4 000 regions of 150 bases, one every 312, groups 0..6 in turn."""
    k = np.arange(REGIONS_PER_CONTIG)
    start = np.tile(k * REGION_STRIDE + 100, N_CONTIG).astype(np.int32)
    group = np.tile(k % (N_CONTIG - 1), N_CONTIG).astype(np.int32)
    return np.arange(N_CONTIG + 1, dtype=np.int64) * REGIONS_PER_CONTIG, start, start + np.int32(REGION_BASES), group


def host_region_key(b, cols):
    """The group of every record by the rule of include/mdx.h mdx_set_strata_regions, in numpy (every contig has the same
    regions): the first region that ends behind pos, if it begins before the record's end."""
    _, start, end, group = cols
    start, end, group = (a[:REGIONS_PER_CONTIG].astype(np.int64) for a in (start, end, group))
    consumes = np.isin(b.cigar & 15, (0, 2, 3, 7, 8))
    span = np.add.reduceat(np.concatenate([np.where(consumes, b.cigar >> 4, 0).astype(np.int64), [0]]), b.cigar_off[:-1].astype(np.int64))
    span[b.cigar_off[1:] == b.cigar_off[:-1]] = 0
    pos = b.pos.astype(np.int64)
    rec_end = pos + np.maximum(1, span)
    at = np.searchsorted(end, pos, side="right")
    hit = (at < REGIONS_PER_CONTIG) & (start[np.minimum(at, REGIONS_PER_CONTIG - 1)] < rec_end) & (b.tid >= 0) & (b.tid < N_CONTIG)
    return np.where(hit, group[np.minimum(at, REGIONS_PER_CONTIG - 1)], N_CONTIG - 1).astype(np.uint16)


def main():
    argv = list(sys.argv[1:])
    out = None
    regions = "--regions" in argv
    if regions:
        argv.remove("--regions")
    if "--out" in argv:
        at = argv.index("--out")
        out = argv[at + 1]
        del argv[at:at + 2]
    n = int(argv[0]) if argv else 16_000_000
    reps = int(argv[1]) if len(argv) > 1 else 9
    ref = synth.make_genome(sizes=tuple(("contig%d" % i, 1_250_000) for i in range(N_CONTIG)))
    # (before the process touches the GPU: the generator forks)
    b = synth.parallel_batch(CONFIG3, ref, n, 3)
    names = list(ref.names)
    with DamageEngine([("s", "l")], 70, 10, 0, lgd_max=4096, groups=names) as ea, \
            DamageEngine([("s", "l%d" % i) for i in range(N_CONTIG)], 70, 10, 0, lgd_max=4096) as eb:
        cols = region_columns() if regions else None

        def set_strata():
            if regions:
                ea.set_strata_regions(*cols)
            else:
                ea.set_strata(np.arange(N_CONTIG))
        set_strata()
        ea.set_reference(ref)
        eb.set_reference(ref)
        b.lib[:] = 0
        da, va = resident_without_sort(ea, b)
        # the same key, made on the host
        b.lib[:] = host_region_key(b, cols) if regions else np.clip(b.tid, 0, N_CONTIG - 1).astype(np.uint16)
        per_group = np.bincount(b.lib, minlength=N_CONTIG).tolist()
        db, vb = resident_without_sort(eb, b)
        for _ in range(2):
            one_call(ea, va)
            one_call(eb, vb)
        ea.reset()
        eb.reset()
        set_strata()
        ta, tb = [], []
        for _ in range(reps):
            ta.append(one_call(ea, va))
            tb.append(one_call(eb, vb))
        sorts = (ea.libsorts(), eb.libsorts())
        got, want = ea.finish(), eb.finish()
        parity = bool((got.strata.mis == want.mis).all() and (got.strata.comp == want.comp).all() and
                      (got.strata.lgd == want.lgd).all() and got.n_kept == want.n_kept and
                      int(got.kept.sum()) == want.n_kept)
        da.free()
        db.free()
    med_a, med_b = float(np.median(ta)), float(np.median(tb))
    spread_b = (max(tb) - min(tb)) / med_b
    ratio = med_a / med_b
    rows = [
        {"what": "strata_cost_regions" if regions else "strata_cost",
         "form": ("region key (%d regions of %d bases per contig, 7 groups and the rest) into a scratch column in front of the launch"
                  % (REGIONS_PER_CONTIG, REGION_BASES)) if regions else "scratch key column in front of the launch",
         "records": n, "contigs": N_CONTIG, "repeats": reps, "records_per_group": per_group,
         "timed": "wall clock of tabulate + sync per call, a and b interleaved in one process", "sorts_in_launch": sorts,
         "parity_a_equals_b": parity},
        {"what": "a: %sstratified context, 1 library x 8 groups" % ("region-" if regions else ""), "ms": [round(x, 3) for x in ta], "median_ms": round(med_a, 3)},
        {"what": "b: plain context, 8 libraries, key in the lib column (baseline)", "ms": [round(x, 3) for x in tb],
         "median_ms": round(med_b, 3), "spread": round(spread_b, 4)},
        {"what": "ratio a / b", "ratio": round(ratio, 4)} if regions else
        {"what": "ratio a / b", "ratio": round(ratio, 4), "bound": round(1.03 + spread_b, 4), "within_bound": bool(ratio <= 1.03 + spread_b)},
    ]
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if out:
        pathlib.Path(out).write_text(text)
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
