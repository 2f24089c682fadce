"""What the strata key costs (include/mdx.h mdx_set_strata): 16 M config-3 records over a genome of 8 contigs, tabulated
(a) by a stratified context of 1 library x 8 groups — the key column made on the device in front of the launch — and
(b) by a plain context of 8 libraries whose lib column was set to the same key on the host: what the library could do
before it had strata, the baseline.  Both over a resident 4-bit batch WITHOUT its bucketed copy (mdx_batch::libsort), as
the views of the file decoders come: the sort by key runs inside every call, in (a) behind the key kernel.  The two are run
interleaved in one process — a, b, a, b, ... — and timed on the wall clock, a call and its synchronisation, so that whatever
the box does to one it does to the other; the spread of (b)'s own repeats is quoted beside the ratio.  The key moves 10
bytes per record (flag, tid and lib in, a key out) against the 240 of the tabulation: a ratio near 1.03 is what the
arithmetic allows.  The two blocks are compared bit for bit on the way.  Run on the GPU box:
    python tools/strata_cost.py [--out FILE] [--regions | --damage] [records] [repeats]
--regions: (a) is a region-stratified context (mdx_set_strata_regions) of 1 library x 8 groups — 4 000 regions of 150 bases
per contig in seven groups and the rest, so the binary search of a sequence's slice takes 12 steps — and (b)'s lib column
holds the same key made on the host with numpy.  The region key reads pos, the two CIGAR offsets and the CIGAR words (one
to three for most records) on top of the 10 bytes of the tid key: some 26 bytes per record, and the search's loads, which
stay in the L2 (384 KB of intervals).  No bound is fixed: the rows say what was seen.
--damage: (a) is a damage-stratified context (mdx_set_strata_damage, one terminal position) of 1 library x 4 groups and (b)
a plain context of 4 libraries whose lib column holds the same key, made on the host with numpy from the rule.  On top of
the tid key's 10 bytes the damage key reads pos, the CIGAR offsets and words, the SEQ offsets and a symbol of SEQ and of the
reference per end — some 40 bytes, in one or two random 128-byte lines each of SEQ and reference per record.  No bound is
fixed here either."""
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


def host_damage_key(b, ref):
    """The group of every record by the rule of include/mdx.h mdx_set_strata_damage for ONE terminal position, double-stranded,
    no --min-basequal, in numpy: the left end is damaged if the first column (the first M I D = X operation) is no gap and
    pairs a read T with a reference C, the right end if the last column is no gap and pairs a read A with a reference G — the
    reference's last column is the span's last base wherever an N shifts the gaps away from the end; a forward read's 5p end
    is its left one, a reverse read's its right one."""
    bases, offs = ref.concat()
    up = np.where((bases >= 97) & (bases <= 122), bases - 32, bases).astype(np.uint8)
    n = b.n
    c0, c1 = b.cigar_off[:-1].astype(np.int64), b.cigar_off[1:].astype(np.int64)
    op, ln = (b.cigar & 15).astype(np.int64), (b.cigar >> 4).astype(np.int64)
    rec = np.repeat(np.arange(n), c1 - c0)
    idx = np.arange(op.shape[0], dtype=np.int64)

    def per_record(values):
        return np.bincount(rec, weights=values, minlength=n).astype(np.int64)

    def first_last(mask):
        big = op.shape[0] + 1
        first = np.full(n, big, np.int64)
        np.minimum.at(first, rec[mask], idx[mask])
        last = np.full(n, -1, np.int64)
        np.maximum.at(last, rec[mask], idx[mask])
        return first, last
    is_col = np.isin(op, (0, 1, 2, 7, 8)) & (ln > 0)
    span = np.maximum(1, per_record(np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0)))
    n_skip, rlen = per_record(np.where(op == 3, ln, 0)), per_record(np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0))
    first_col, last_col = first_last(is_col)
    first_aln, last_aln = first_last(~np.isin(op, (4, 5)))
    soft = np.where(op == 4, ln, 0)
    lead = per_record(np.where(idx < first_aln[rec], soft, 0))
    trail = per_record(np.where((idx > last_aln[rec]) & (idx > c0[rec]), soft, 0))
    s0, s1 = b.seq_off[:-1].astype(np.int64), b.seq_off[1:].astype(np.int64)
    qs, qe = lead, (s1 - s0) - trail
    has = (last_col >= 0) & (qe > qs)
    pos, tid = b.pos.astype(np.int64), np.clip(b.tid, 0, len(ref.names) - 1).astype(np.int64)
    ok = has & (b.tid >= 0) & (b.tid < len(ref.names)) & (pos >= 0) & (pos + span <= offs[tid + 1] - offs[tid])
    safe = np.where(ok, 1, 0)
    op_first, op_last = op[np.minimum(first_col, op.shape[0] - 1)], op[np.maximum(last_col, 0)]
    read_l, read_r = b.seq[(s0 + qs) * safe], b.seq[(s0 + qe - 1) * safe]
    ref_l, ref_r = up[(offs[tid] + pos) * safe], up[(offs[tid] + pos + span - 1) * safe]
    left = ok & ~np.isin(op_first, (1, 2)) & (read_l == ord("T")) & (ref_l == ord("C"))
    ref_gap_r = (op_last == 1) & (n_skip == 0) & (rlen > 0)
    right = ok & (op_last != 2) & ~ref_gap_r & (read_r == ord("A")) & (ref_r == ord("G"))
    rev = (b.flag & 0x10) != 0
    p5, p3 = np.where(rev, right, left), np.where(rev, left, right)
    return (p5.astype(np.uint16) + 2 * p3.astype(np.uint16)).astype(np.uint16)


def main():
    argv = list(sys.argv[1:])
    out = None
    regions = "--regions" in argv
    if regions:
        argv.remove("--regions")
    damage = "--damage" in argv
    if damage:
        argv.remove("--damage")
    if "--out" in argv:
        at = argv.index("--out")
        out = argv[at + 1]
        del argv[at:at + 2]
    n = int(argv[0]) if argv else 16_000_000
    reps = int(argv[1]) if len(argv) > 1 else 9
    ref = synth.make_genome(sizes=tuple(("contig%d" % i, 1_250_000) for i in range(N_CONTIG)))
    # (before the process touches the GPU: the generator forks)
    b = synth.parallel_batch(CONFIG3, ref, n, 3)
    names = list(DamageEngine.DAMAGE_GROUPS) if damage else list(ref.names)
    with DamageEngine([("s", "l")], 70, 10, 0, lgd_max=4096, groups=names) as ea, \
            DamageEngine([("s", "l%d" % i) for i in range(len(names))], 70, 10, 0, lgd_max=4096) as eb:
        cols = region_columns() if regions else None

        def set_strata():
            if damage:
                ea.set_strata_damage(1)
            elif regions:
                ea.set_strata_regions(*cols)
            else:
                ea.set_strata(np.arange(N_CONTIG))
        # (the damage key reads the reference: in place before the strata, which upload keys by)
        ea.set_reference(ref)
        eb.set_reference(ref)
        set_strata()
        b.lib[:] = 0
        da, va = resident_without_sort(ea, b)
        # the same key, made on the host
        b.lib[:] = host_damage_key(b, ref) if damage else host_region_key(b, cols) if regions else np.clip(b.tid, 0, N_CONTIG - 1).astype(np.uint16)
        per_group = np.bincount(b.lib, minlength=len(names)).tolist()
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
        {"what": "strata_cost_damage" if damage else "strata_cost_regions" if regions else "strata_cost",
         "form": "damage key (one terminal position, double-stranded) into a scratch column in front of the launch" if damage else ("region key (%d regions of %d bases per contig, 7 groups and the rest) into a scratch column in front of the launch"
                  % (REGIONS_PER_CONTIG, REGION_BASES)) if regions else "scratch key column in front of the launch",
         "records": n, "contigs": N_CONTIG, "repeats": reps, "records_per_group": per_group,
         "timed": "wall clock of tabulate + sync per call, a and b interleaved in one process", "sorts_in_launch": sorts,
         "parity_a_equals_b": parity},
        {"what": "a: %sstratified context, 1 library x %d groups" % ("damage-" if damage else "region-" if regions else "", len(names)), "ms": [round(x, 3) for x in ta], "median_ms": round(med_a, 3)},
        {"what": "b: plain context, %d libraries, key in the lib column (baseline)" % len(names), "ms": [round(x, 3) for x in tb],
         "median_ms": round(med_b, 3), "spread": round(spread_b, 4)},
        {"what": "ratio a / b", "ratio": round(ratio, 4)} if regions or damage else
        {"what": "ratio a / b", "ratio": round(ratio, 4), "bound": round(1.03 + spread_b, 4), "within_bound": bool(ratio <= 1.03 + spread_b)},
    ]
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if out:
        pathlib.Path(out).write_text(text)
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
