"""Helpers of the PMD-score tests (``--by-pmd-score``, include/mdx.h ``mdx_set_strata_pmd``): a restatement of the rule in
Python that shares nothing with the product — it builds the two gapped strings of every record in its true alignment and
walks their columns — and the records the tests run on.

The rule, as the feature's issue words it.  The query is SEQ without its terminal soft clips (hard clips ignored), ``nq``
bases ``q = 0 .. nq-1`` in the record's orientation; forward ``z5 = q+1, z3 = nq-q``, reverse (0x10) ``z5 = nq-q, z3 = q+1``;
insertions are query bases (they move z and add no term), deletions and N are none.  Only columns of M, =, X add terms,
reference base R under read base B, exact symbols: in the molecule's orientation (a reverse read complemented) a 5p term
at z5 where R = C and B in {C, T}, a 3p term at z3 where R = G and B in {G, A} (single-stranded: R = C, B in {C, T}); B = R is
a match.  ``D_z = p (1-p)^(z-1) + C`` for z = 1..256, beyond that ``D_256``; ``eps_q = 10^(-q/10) / 3`` for q = 0..93,
larger bytes are 93, and eps = 0 for a record without qualities (no column, or a first byte of 0xFF);
``Pm(D) = (1-D)(1-eps)(1-pi) + D eps (1-pi) + eps pi (1-D)``, ``match = log(Pm(D_z) / Pm(0))``,
``mismatch = log((1-Pm(D_z)) / (1-Pm(0)))``; every term is ``round(ldexp(term, 24))`` and a record's score S their int64
sum; its group the number of thresholds with ``S >= ceil(t 2^24)``; its histogram bin ``clamp((S >> 23) + 41, 0, 81)``.  A
tid outside the reference, a pos < 0 or a window beyond its sequence: S = 0."""

import functools
import math

import numpy as np

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULT_MODEL = (0.3, 0.01, 0.001)


def double_terms(z, q, model=DEFAULT_MODEL):
    """(match, mismatch) as doubles for distance ``z`` (1-based, any) and quality column ``q`` (94: eps = 0)."""
    p, C, pi = model
    eps = 10 ** (-q / 10) / 3 if q < 94 else 0.0
    z = min(z, 256)
    D = p * (1 - p) ** (z - 1) + C

    def pm(D):
        return (1 - D) * (1 - eps) * (1 - pi) + D * eps * (1 - pi) + eps * pi * (1 - D)
    return math.log(pm(D) / pm(0.0)), math.log((1 - pm(D)) / (1 - pm(0.0)))


@functools.lru_cache(maxsize=None)
def restated_table(model=DEFAULT_MODEL):
    """int [2][256][95] of the restatement: Python ints in nested lists (no numpy in the arithmetic)."""
    out = [[[0] * 95 for _ in range(256)] for _ in range(2)]
    for z in range(1, 257):
        for q in range(95):
            m, x = double_terms(z, q, model)
            out[0][z - 1][q] = round(math.ldexp(m, 24))
            out[1][z - 1][q] = round(math.ldexp(x, 24))
    return out


def gapped(ops, seq):
    """The two gapped strings of a record over its query: (read string, reference index per column or None).  The read
    string holds the query's bases and '-' under deleted or skipped reference bases; the reference column is None ('-')
    over an insertion or a soft clip inside the query."""
    real = [(op, ln) for op, ln in ops if op != 5]
    lead = 0
    for op, ln in real:
        if op != 4:
            break
        lead += ln
    trail = 0
    # (as the product's other keys take it: a trailing clip is not looked for in the CIGAR's first operation)
    for k in range(len(ops) - 1, 0, -1):
        op, ln = ops[k]
        if op == 5:
            continue
        if op != 4:
            break
        trail += ln
    query = seq[lead:len(seq) - trail] if len(seq) - trail > lead else ""
    read, ref_at = [], []
    x, r = 0, 0
    for op, ln in ops:
        for _ in range(ln):
            if op in (0, 7, 8, 1, 4):
                q = x - lead
                if 0 <= q < len(query):
                    read.append(query[q])
                    ref_at.append(r if op in (0, 7, 8) else None)
                x += 1
                if op in (0, 7, 8):
                    r += 1
            elif op in (2, 3):
                read.append("-")
                ref_at.append(r)
                r += 1
    return query, lead, read, ref_at


def score_record(ops, seq, qual, flag, window, single_stranded=False, model=DEFAULT_MODEL, want_doubles=False):
    """S of one record.  ``seq``: str; ``qual``: sequence of ints over SEQ, or None; ``window``: the upper-cased reference
    bases under the record (str), or None for a record whose tid or window lies outside the reference.
    ``want_doubles``: (S, [the doubles of its terms]) instead."""
    table = restated_table(tuple(model))
    if window is None:
        return (0, []) if want_doubles else 0
    query, lead, read, ref_at = gapped(ops, seq)
    has_qual = qual is not None and len(seq) > 0 and int(qual[0]) != 0xFF
    nq = len(query)
    reverse = bool(flag & 0x10)
    total, doubles = 0, []
    q = -1
    for base, r in zip(read, ref_at):
        if base == "-":
            continue                    # a deleted or skipped reference base: no query base
        q += 1
        if r is None or r >= len(window):
            continue                    # an insertion (or a clip inside the query): a query base, no term
        R, B = window[r], base
        if reverse:
            R, B = COMPLEMENT.get(R), COMPLEMENT.get(B)
        if R is None or B is None:
            continue
        z5, z3 = (nq - q, q + 1) if reverse else (q + 1, nq - q)
        col = min(int(qual[lead + q]), 93) if has_qual else 94
        hits = []
        if R == "C" and B in "CT":
            hits.append((z5, B == "T"))
        if single_stranded:
            if R == "C" and B in "CT":
                hits.append((z3, B == "T"))
        elif R == "G" and B in "GA":
            hits.append((z3, B == "A"))
        for z, mismatch in hits:
            total += table[1 if mismatch else 0][min(z, 256) - 1][col]
            if want_doubles:
                doubles.append(double_terms(z, col, tuple(model))[1 if mismatch else 0])
    return (total, doubles) if want_doubles else total


def window_of(ref, tid, pos, ops):
    """The upper-cased reference bases under a record, or None for a degenerate one."""
    span = max(1, sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8)))
    if tid < 0 or tid >= len(ref.names) or pos < 0 or pos + span > len(ref.seqs[tid]):
        return None
    return ref.seqs[tid][pos:pos + span].decode("latin-1").upper()


def scores(ref, b, single_stranded=False, model=DEFAULT_MODEL):
    """int64 [n]: S of every record of a batch."""
    out = np.zeros(b.n, np.int64)
    for i in range(b.n):
        c0, c1, s0, s1 = int(b.cigar_off[i]), int(b.cigar_off[i + 1]), int(b.seq_off[i]), int(b.seq_off[i + 1])
        ops = [(int(w) & 15, int(w) >> 4) for w in b.cigar[c0:c1]]
        seq = b.seq[s0:s1].tobytes().decode("latin-1")
        qual = None if b.qual is None else b.qual[s0:s1]
        out[i] = score_record(ops, seq, qual, int(b.flag[i]), window_of(ref, int(b.tid[i]), int(b.pos[i]), ops), single_stranded, model)
    return out


def threshold_fx(t):
    return math.ceil(math.ldexp(float(t), 24))


def groups_of(S, thresholds):
    return np.sum([S >= threshold_fx(t) for t in thresholds], axis=0).astype(np.int64)


def bins_of(S):
    return np.clip((S >> 23) + 41, 0, 81).astype(np.int64)


def histogram(b, S, n_libraries):
    """uint64 [n_libraries][82] of the kept records."""
    keep = ((b.flag & 0xF04) == 0) & (b.lib < n_libraries)
    return np.bincount(b.lib[keep].astype(np.int64) * 82 + bins_of(S[keep]), minlength=n_libraries * 82).astype(np.uint64).reshape(n_libraries, 82)


def scores_tsv(libraries, hist):
    """``by_pmd/scores.tsv`` written down once more: the libraries sorted, 82 bins each, the ends open."""
    edges = ["-inf"] + ["%g" % (-20 + k / 2) for k in range(81)] + ["inf"]
    rows = ["Sample\tLibrary\tLow\tHigh\tReads"]
    for (sample, library), li in sorted((tuple(lib), i) for i, lib in enumerate(libraries)):
        rows += ["%s\t%s\t%s\t%s\t%d" % (sample, library, edges[k], edges[k + 1], int(hist[li][k])) for k in range(82)]
    return "\n".join(rows) + "\n"


def group_names(thresholds):
    ts = ["%g" % t for t in thresholds]
    return ["<" + ts[0]] + ["[%s,%s)" % (ts[k], ts[k + 1]) for k in range(len(ts) - 1)] + [">=" + ts[-1]]


# ---------------------------------------------------------------------- records
def _cigar(text):
    from mapdamage_amd import synth
    return synth._parse_cigar(text) if text else []


# name, tid, pos, CIGAR, flag, what the read holds ("ref": the reference along the alignment with C>T / G>A put in at both
# ends; or a literal SEQ), qualities (None, an int for all, or a list)
HAND = [
    ("every operation", 0, 300, "3H2S10M2I5M3D4M20N6=3X2P4M2S1H", 0, "ref", 30),
    ("every operation -", 0, 400, "3H2S10M2I5M3D4M20N6=3X2P4M2S1H", 16, "ref", 30),
    ("clips", 0, 500, "5S30M4S", 0, "ref", 25),
    ("hard and soft clips -", 0, 600, "2H5S30M4S3H", 16, "ref", 25),
    ("only a clip in front", 0, 650, "6S30M", 0, "ref", 25),
    ("ins first", 0, 700, "2I30M", 0, "ref", 30),
    ("ins last", 0, 800, "30M2I", 0, "ref", 30),
    ("ins first -", 0, 900, "2I30M", 16, "ref", 30),
    ("del first", 0, 1000, "2D30M", 0, "ref", 30),
    ("del last", 0, 1100, "30M2D", 0, "ref", 30),
    ("del behind the first base -", 0, 1200, "1M2D30M", 16, "ref", 30),
    ("N", 0, 1300, "20M50N10M", 0, "ref", 30),
    ("N -", 0, 1400, "2M50N28M", 16, "ref", 30),
    ("one base", 1, 100, "1M", 0, "ref", 30),
    ("one base -", 1, 101, "1M", 16, "ref", 30),
    ("255 bases", 1, 200, "255M", 0, "ref", 30),
    ("256 bases", 1, 500, "256M", 16, "ref", 30),
    ("257 bases", 1, 800, "257M", 0, "ref", 30),
    ("600 bases", 0, 2000, "600M", 0, "ref", 30),
    ("600 bases -", 0, 2700, "300M5I295M", 16, "ref", 30),
    ("no qualities", 1, 1200, "40M", 0, "ref", None),
    ("no qualities -", 1, 1300, "40M", 16, "ref", None),
    ("qualities 0", 1, 1400, "40M", 0, "ref", 0),
    ("qualities 93", 1, 1500, "40M", 0, "ref", 93),
    ("qualities 200", 1, 1600, "40M", 16, "ref", 200),
    ("qualities mixed", 1, 1700, "40M", 0, "ref", [0, 93, 200, 94, 254, 2, 41] * 5 + [30] * 5),
    ("read N and ambiguity codes", 2, 100, "12M", 0, "NRYCTGAMKNNT", 30),
    ("lower-case read", 2, 200, "30M", 0, "lower", 30),
    ("soft-masked reference", 0, 6000, "40M", 0, "ref", 30),
    ("reference N run", 0, 2990, "60M", 0, "ref", 30),
    ("many operations", 3, 100, "3M1I3M1D3M1I3M1D3M1I3M1D3M1I3M1D3M1I3M", 0, "ref", 30),
    ("many operations -", 3, 300, "2S3M1I3M1D3M1I3M1D3M1I3M1D3M1I3M1D3M1I3M2S", 16, "ref", 30),
    ("nine operations", 3, 500, "5M1I5M1D5M1I5M1D5M", 0, "ref", 30),
    ("eight operations", 3, 600, "5M1I5M1D5M1I5M1D", 0, "ref", 30),
    ("position 0", 1, 0, "30M", 0, "ref", 30),
    ("ends at the last base", 3, 2470, "30M", 16, "ref", 30),
    ("unmapped", -1, -1, "", 4, "", None),
]
# degenerate records: S = 0, and the tabulation reports them if they are kept
DEGENERATE = [
    ("tid outside the reference", 9, 100, "30M", 0, "ACGT" * 7 + "AC", 30),
    ("negative position", 0, -5, "30M", 0, "ACGT" * 7 + "AC", 30),
    ("window past the contig's end", 4, 1990, "30M", 0, "CCCC" * 7 + "CC", 30),
    ("window past the contig's end by its deletion", 4, 1965, "30M10D", 0, "CCCC" * 7 + "CC", 30),
]


def _hand_record(ref, i, name, tid, pos, cigar, flag, content, qual, drop=False):
    ops = _cigar(cigar)
    n_query = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
    if content in ("ref", "lower"):
        contig = ref.seqs[tid].decode("latin-1").upper()
        seq, r = [], pos
        for op, ln in ops:
            if op in (0, 7, 8):
                seq.extend(contig[r:r + ln])
                r += ln
            elif op in (1, 4):
                seq.extend("C" * ln)
            elif op in (2, 3):
                r += ln
        # deamination at both ends of the molecule: C>T within three aligned bases of the left end, G>A of the right one
        # (these are the record's own ends: a reverse record shows the same substitutions, which then count against it)
        for k in list(range(min(4, len(seq)))) + list(range(max(0, len(seq) - 4), len(seq))):
            if seq[k] == "C" and k < 4 and k % 2 == 0:
                seq[k] = "T"
            elif seq[k] == "G" and k >= len(seq) - 4 and k % 2 == 1:
                seq[k] = "A"
        seq = "".join(seq)
        if content == "lower":
            seq = seq.lower()
    else:
        seq = content
    assert len(seq) == n_query, name
    q = None if qual is None else ([qual] * len(seq) if isinstance(qual, int) else list(qual))
    return dict(flag=flag | (0x200 if drop else 0), lib=i % 2, tid=tid, pos=pos, cigar=ops, seq=seq, qual=q)


def hand_batch(ref, degenerate="dropped"):
    """The hand-made records over ``tests.test_gpu_strata.genome5()``; ``degenerate``: "kept" (the host build: a kept
    degenerate record scores 0), "dropped" (the device: flag 0x200, for the tabulation reports a kept one) or "none"."""
    from mapdamage_amd.batch import batch_from_records
    rows = [_hand_record(ref, i, *row) for i, row in enumerate(HAND)]
    if degenerate != "none":
        rows += [_hand_record(ref, i, *row, drop=degenerate == "dropped") for i, row in enumerate(DEGENERATE)]
    return batch_from_records(rows, with_qual=True)


def synthetic_batch(ref, n, seed, nlib, len_range=(30, 160), with_qual=True):
    """``n`` mixed records with every kind of operation, 3 % of them dropped by the flag filter, damaged as the default
    model says (synth._damage_probs: 0.3 x 0.7^i + 0.01), their qualities spread over 2 .. 41."""
    from mapdamage_amd import synth
    from tests.test_gpu_strata import MIXED
    b = synth.make_reads(ref, n, seed, nlib=nlib, with_qual=with_qual, **dict(MIXED, len_range=len_range))
    if with_qual:
        rng = np.random.default_rng(seed + 1)
        nb = b.seq.shape[0]
        b.qual = np.where(rng.random(nb) < 0.2, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    return b


def pack4(seq):
    from tests.damage_util import pack4 as p4
    return p4(seq)
