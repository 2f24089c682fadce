"""What the strata key costs (include/mdx.h mdx_set_strata): 16 M config-3 records over a genome of 8 contigs, tabulated
(a) by a stratified context of 1 library x 8 groups — the key column made on the device in front of the launch — and
(b) by a plain context of 8 libraries whose lib column was set to the same key on the host: what the library could do
before it had strata, the baseline.  Both over a resident 4-bit batch WITHOUT its bucketed copy (mdx_batch::libsort), as
the views of the file decoders come: the sort by key runs inside every call, in (a) behind the key kernel.  The two are run
interleaved in one process — a, b, a, b, ... — and timed on the wall clock, a call and its synchronisation, so that whatever
the box does to one it does to the other; the spread of (b)'s own repeats is quoted beside the ratio.  The key moves 10
bytes per record (flag, tid and lib in, a key out) against the 240 of the tabulation: a ratio near 1.03 is what the
arithmetic allows.  The two blocks are compared bit for bit on the way.  Run on the GPU box:
    python tools/strata_cost.py [--out FILE] [--regions | --damage | --pmd] [records] [repeats]
--regions: (a) is a region-stratified context (mdx_set_strata_regions) of 1 library x 8 groups — 4 000 regions of 150 bases
per contig in seven groups and the rest, so the binary search of a sequence's slice takes 12 steps — and (b)'s lib column
holds the same key made on the host with numpy.  The region key reads pos, the two CIGAR offsets and the CIGAR words (one
to three for most records) on top of the 10 bytes of the tid key: some 26 bytes per record, and the search's loads, which
stay in the L2 (384 KB of intervals).  No bound is fixed: the rows say what was seen.
--damage: (a) is a damage-stratified context (mdx_set_strata_damage, one terminal position) of 1 library x 4 groups and (b)
a plain context of 4 libraries whose lib column holds the same key, made on the host with numpy from the rule.  On top of
the tid key's 10 bytes the damage key reads pos, the CIGAR offsets and words, the SEQ offsets and a symbol of SEQ and of the
reference per end — some 40 bytes, in one or two random 128-byte lines each of SEQ and reference per record.  No bound is
fixed here either.
--pmd: the records carry qualities; (a) is a PMD-stratified context (mdx_set_strata_pmd, thresholds 0 and 3, the default
model) of 1 library x 3 groups, (a') the same context with the trivial key kernel — a lane per record, MDX_PMD_LANE=1 —
instead of the cooperative one, (a'') the cooperative kernel with every term read from global memory instead of part of the
table kept in the LDS (MDX_PMD_NO_LDS=1), and (b) a plain context of 3 libraries whose lib column holds the same key, made on
the host by the rule's header compiled for the host (csrc/mdx_pmd_key.h through tests/pmd_key_host.cpp, which
tests/test_pmd.py holds to the rule's restatement: this mode needs a host C++ compiler where it runs, and that file of the
tests).  A repeat is a, b, a', b, a'', b — every timed call behind a call of the other context; the first b of a repeat is
the timed one, the other two keep (b)'s tables in step with (a)'s for the comparison of the blocks.  The key reads every aligned base: the 4-bit SEQ, the
QUAL bytes and the reference window of a record, some 250 bytes on top of the fixed columns — as much again as the
tabulation streams; the rows give the key kernels' own time (a - b, a' - b), the bytes they move and what that is of an
8 TB/s roofline.  No bound is fixed."""
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


def host_pmd_key(b, ref, thresholds, workdir):
    """(group, histogram bin) of every record by csrc/mdx_pmd_key.h compiled for the host (the default model, double-stranded)."""
    import subprocess
    from mapdamage_amd import pmd
    so = pathlib.Path(workdir) / "pmd_key_host.so"
    subprocess.check_call(["c++", "-O2", "-shared", "-fPIC", "-I", str(ROOT / "mapdamage_amd" / "csrc"),
                           str(ROOT / "tests" / "pmd_key_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    bases, offs = ref.concat()
    up = np.where((bases >= 97) & (bases <= 122), bases - 32, bases).astype(np.uint8)
    resident = np.where(np.isin(up, np.frombuffer(b"ACGT", np.uint8)), up, np.uint8(0x85)).astype(np.uint8)
    offs = np.ascontiguousarray(offs, np.int64)
    terms = np.ascontiguousarray(pmd.term_table())
    fx = np.array([pmd.threshold_fx(t) for t in thresholds], np.int64)
    score, group = np.zeros(b.n, np.int64), np.zeros(b.n, np.uint8)
    bins, noq = np.zeros(b.n, np.uint8), np.zeros(b.n, np.uint8)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    lib.pmd_scores_host(ctypes.c_int64(b.n), ctypes.c_int64(b.cigar.shape[0]), ctypes.c_int64(b.seq.shape[0]), ptr(b.flag), ptr(b.tid),
                        ptr(b.pos), ptr(b.cigar_off), ptr(b.cigar), ptr(b.seq_off), ptr(b.seq), ptr(b.qual), 0, ptr(resident), ptr(offs),
                        len(ref.names), 0, ptr(terms), len(thresholds), ptr(fx), 1, ptr(score), ptr(group), ptr(bins), ptr(noq))
    return group.astype(np.uint16), bins


PMD_THRESHOLDS = (0.0, 3.0)


def main():
    argv = list(sys.argv[1:])
    out = None
    regions = "--regions" in argv
    if regions:
        argv.remove("--regions")
    damage = "--damage" in argv
    if damage:
        argv.remove("--damage")
    by_pmd = "--pmd" in argv
    if by_pmd:
        argv.remove("--pmd")
    if "--out" in argv:
        at = argv.index("--out")
        out = argv[at + 1]
        del argv[at:at + 2]
    n = int(argv[0]) if argv else 16_000_000
    reps = int(argv[1]) if len(argv) > 1 else 9
    ref = synth.make_genome(sizes=tuple(("contig%d" % i, 1_250_000) for i in range(N_CONTIG)))
    # (before the process touches the GPU: the generator forks)
    b = synth.parallel_batch(dict(CONFIG3, with_qual=True) if by_pmd else CONFIG3, ref, n, 3)
    names = ["<0", "[0,3)", ">=3"] if by_pmd else list(DamageEngine.DAMAGE_GROUPS) if damage else list(ref.names)
    if by_pmd:
        import os
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            pmd_key, pmd_bins = host_pmd_key(b, ref, PMD_THRESHOLDS, tmp)
    with DamageEngine([("s", "l")], 70, 10, 0, lgd_max=4096, groups=names) as ea, \
            DamageEngine([("s", "l%d" % i) for i in range(len(names))], 70, 10, 0, lgd_max=4096) as eb:
        cols = region_columns() if regions else None

        def set_strata():
            if by_pmd:
                ea.set_strata_pmd(PMD_THRESHOLDS)
            elif damage:
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
        b.lib[:] = pmd_key if by_pmd else host_damage_key(b, ref) if damage else host_region_key(b, cols) if regions else np.clip(b.tid, 0, N_CONTIG - 1).astype(np.uint16)
        per_group = np.bincount(b.lib, minlength=len(names)).tolist()
        db, vb = resident_without_sort(eb, b)
        for _ in range(2):
            one_call(ea, va)
            one_call(eb, vb)
        ea.reset()
        eb.reset()
        set_strata()
        ta, tb, tl, tn = [], [], [], []
        for _ in range(reps):
            ta.append(one_call(ea, va))
            tb.append(one_call(eb, vb))
            if by_pmd:
                # (a'), (a''): the same context and batch through the other two kernels; their counts go to the same tables,
                # so (b) is called behind each, untimed, and the parity below is taken over a + a' + a'' against b three times
                for knob, times in (("MDX_PMD_LANE", tl), ("MDX_PMD_NO_LDS", tn)):
                    os.environ[knob] = "1"
                    times.append(one_call(ea, va))
                    del os.environ[knob]
                    one_call(eb, vb)
        sorts = (ea.libsorts(), eb.libsorts())
        got, want = ea.finish(), eb.finish()
        hist_ok = True
        if by_pmd:
            hist_ok = bool((got.pmd_hist[0] == 3 * reps * np.bincount(pmd_bins[(b.flag & 0xF04) == 0], minlength=82)).all())
        parity = bool((got.strata.mis == want.mis).all() and (got.strata.comp == want.comp).all() and
                      (got.strata.lgd == want.lgd).all() and got.n_kept == want.n_kept and
                      int(got.kept.sum()) == want.n_kept and hist_ok)
        da.free()
        db.free()
    med_a, med_b = float(np.median(ta)), float(np.median(tb))
    spread_b = (max(tb) - min(tb)) / med_b
    ratio = med_a / med_b
    if by_pmd:
        med_l, med_n = float(np.median(tl)), float(np.median(tn))
        # what the key kernel streams: the fixed columns (flag, lib, tid, pos, two offsets in, the key out), the CIGAR words,
        # 4-bit SEQ, QUAL, and a reference byte per reference base of the alignment
        op, ln = b.cigar & 15, (b.cigar >> 4).astype(np.int64)
        key_bytes = 22 * n + 4 * int(b.cigar.shape[0]) + int(b.seq.shape[0]) // 2 + int(b.seq.shape[0]) + int(ln[np.isin(op, (0, 2, 3, 7, 8))].sum())

        def kernel_row(what, med):
            own = med - med_b
            return {"what": what, "ms": round(own, 3), "bytes_per_record": round(key_bytes / n, 1),
                    "TB_per_s": round(key_bytes / (own * 1e-3) / 1e12, 3) if own > 0 else None,
                    "of_8_TB_per_s_roofline": round(key_bytes / (own * 1e-3) / 8e12, 3) if own > 0 else None}
    rows = [
        {"what": "strata_cost_pmd" if by_pmd else "strata_cost_damage" if damage else "strata_cost_regions" if regions else "strata_cost",
         "form": "PMD key (thresholds 0 and 3, default model, double-stranded, records with qualities) into a scratch column in front of the launch" if by_pmd else "damage key (one terminal position, double-stranded) into a scratch column in front of the launch" if damage else ("region key (%d regions of %d bases per contig, 7 groups and the rest) into a scratch column in front of the launch"
                  % (REGIONS_PER_CONTIG, REGION_BASES)) if regions else "scratch key column in front of the launch",
         "records": n, "contigs": N_CONTIG, "repeats": reps, "records_per_group": per_group,
         "timed": "wall clock of tabulate + sync per call, a and b interleaved in one process", "sorts_in_launch": sorts,
         "parity_a_equals_b": parity},
        {"what": "a: %sstratified context, 1 library x %d groups" % ("PMD-" if by_pmd else "damage-" if damage else "region-" if regions else "", len(names)), "ms": [round(x, 3) for x in ta], "median_ms": round(med_a, 3)},
        {"what": "b: plain context, %d libraries, key in the lib column (baseline)" % len(names), "ms": [round(x, 3) for x in tb],
         "median_ms": round(med_b, 3), "spread": round(spread_b, 4)},
        {"what": "ratio a / b", "ratio": round(ratio, 4)} if regions or damage or by_pmd else
        {"what": "ratio a / b", "ratio": round(ratio, 4), "bound": round(1.03 + spread_b, 4), "within_bound": bool(ratio <= 1.03 + spread_b)},
    ]
    if by_pmd:
        rows += [{"what": "a': the same context, trivial key kernel (a lane per record, MDX_PMD_LANE=1)", "ms": [round(x, 3) for x in tl],
                  "median_ms": round(med_l, 3)},
                 {"what": "ratio a' / b", "ratio": round(med_l / med_b, 4)},
                 {"what": "a'': the same context, cooperative key kernel with every term from global memory (MDX_PMD_NO_LDS=1)",
                  "ms": [round(x, 3) for x in tn], "median_ms": round(med_n, 3)},
                 {"what": "ratio a'' / b", "ratio": round(med_n / med_b, 4)},
                 kernel_row("key kernel alone, cooperative (16 lanes per record), match terms of 128 distances x 48 qualities in the LDS: median a - median b", med_a),
                 kernel_row("key kernel alone, cooperative, every term from global memory: median a'' - median b", med_n),
                 kernel_row("key kernel alone, trivial (a lane per record): median a' - median b", med_l)]
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if out:
        pathlib.Path(out).write_text(text)
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
