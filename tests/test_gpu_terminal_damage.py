"""Strata by terminal damage on the device: tables per (library, none | 5p | 3p | both) from one pass (include/mdx.h
``mdx_set_strata_damage``; ``--by-terminal-damage``, ``--terminal-positions``).

The yardstick shares nothing with the product.  A record's group is read from the reference-pinned CPU oracle run on that
record alone (tests/damage_util.py): 5p-damaged iff its 5p table counts C>T below the terminal positions, 3p-damaged iff its
3p table counts G>A there.  The group tables are tests/test_gpu_regions.py's ``yardstick`` — one oracle run per stratum,
every other record flagged 0x4 — and the comparison is tests/test_gpu_strata.py's ``check``: tables bit for bit, the three
texts byte for byte, the merged block equal to the oracle over the untouched batch."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import layout as L
from mapdamage_amd import synth
from mapdamage_amd.batch import batch_from_records
from tests import damage_util as D
from tests.test_gpu_regions import brute_kept, run, yardstick
from tests.test_gpu_strata import A, CLI_LIBS, FILES, RGS, batch4, check, genome4, genome5, libraries, tree
from tests.util import oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def has_op(b, op):
    return np.asarray([bool(((b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])] & 15) == op).any()) for i in range(b.n)])


def terminal_soft_clip(b):
    """Records whose first or last operation that is no hard clip is a soft clip."""
    out = np.zeros(b.n, bool)
    for i in range(b.n):
        ops = [int(c) & 15 for c in b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])] if int(c) & 15 != 5]
        out[i] = bool(ops) and (ops[0] == 4 or ops[-1] == 4)
    return out


# ---------------------------------------------------------------------- 1. the grid
GRID = [(0, 1), (0, 3), (20, 1), (20, 3)]        # (minqual, terminal positions)


@functools.lru_cache(maxsize=None)
def grid_is_sound():
    """What the comparison needs of the batch before it is trusted: every library x group cell filled, records that change
    group under -Q 20, damaged records with an N operation and with a soft clip at an end."""
    b = D.grid_batch()
    kept = (b.flag & 0xF04) == 0
    assert int(kept.sum()) == 3875
    for minqual, k in GRID:
        cells = brute_kept(b, D.groups_of(D.grid_first(minqual), k), 3, 4)
        assert cells.min() >= 1, (minqual, k, cells)
    for k in (1, 3):
        moved = kept & (D.groups_of(D.grid_first(0), k) != D.groups_of(D.grid_first(20), k))
        assert moved.sum() >= 1, k
    damaged = kept & (D.groups_of(D.grid_first(0), 3) > 0)
    assert (damaged & has_op(b, 3)).sum() >= 1 and (damaged & terminal_soft_clip(b)).sum() >= 1
    for strand in (0, 0x10):
        assert set(D.groups_of(D.grid_first(0), 3)[kept & ((b.flag & 0x10) == strand)]) == {0, 1, 2, 3}
    return True


@functools.lru_cache(maxsize=None)
def want_grid(length, minqual, k, single_stranded=False):
    b, libs = D.grid_batch(), libraries(3)
    group = D.groups_of(D.grid_first(minqual), k, single_stranded)
    groups, kept = yardstick(genome5(), b, libs, group, 4, length, minqual)
    np.testing.assert_array_equal(kept, brute_kept(b, group, 3, 4))
    return groups, kept, oracle_tableset(genome5(), b, libs, length, A, minqual)


def damage_engine(libs, length, minqual, k, single_stranded=False, **kw):
    from mapdamage_amd.engine import DamageEngine
    eng = DamageEngine(libs, length, A, minqual, groups=D.GROUPS, **kw)
    eng.set_strata_damage(k, single_stranded)
    return eng


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("form", ["packed", "ascii", "resident"])
@pytest.mark.parametrize("length,minqual", [(70, 0), (70, 20), (700, 20)])
def test_grid(length, minqual, form, k):
    assert grid_is_sound()
    b = D.grid_batch()
    with damage_engine(libraries(3), length, minqual, k) as eng:
        assert eng.table_mode == ("global" if length == 700 else "lds")
        eng.set_reference(genome5())
        lib_before = b.lib.copy()
        run(eng, b, form)
        if length == 70:
            assert eng.packed_launches() == (0 if form == "ascii" else 1)
        got = eng.finish()
        np.testing.assert_array_equal(b.lib, lib_before)
    assert got.groups == D.GROUPS
    check(got, *want_grid(length, minqual, k))


def test_grid_single_stranded():
    """The 3p criterion is C>T at the 3p positions."""
    assert grid_is_sound()
    first = D.grid_first(0)
    assert (D.groups_of(first, 3, True) != D.groups_of(first, 3, False)).sum() > 100
    with damage_engine(libraries(3), 70, 0, 3, single_stranded=True) as eng:
        eng.set_reference(genome5())
        run(eng, D.grid_batch(), "packed")
        got = eng.finish()
    check(got, *want_grid(70, 0, 3, True))


def test_a_callers_own_4bit_batch_with_qualities_is_folded_in_front_of_the_launch():
    """A resident MDX_SEQ_4BIT batch with its quality column and no bucketed copy (as tools/strata_cost.py
    ``resident_without_sort`` makes the view), under -Q 20: the key is made from the column as the caller brings it, the
    mask is folded and the records are bucketed inside the call."""
    from mapdamage_amd.engine import DamageEngine
    assert grid_is_sound()
    b = D.grid_batch()
    # (uploaded by a context without a threshold: the column stays MDX_SEQ_4BIT and the qualities travel with it)
    with DamageEngine(libraries(3), 70, A, 0) as plain, damage_engine(libraries(3), 70, 20, 3) as eng:
        db = plain.upload(b, packed=True)
        view = type(db.dev)()
        ctypes.memmove(ctypes.byref(view), ctypes.byref(db.dev), ctypes.sizeof(view))
        view.libsort = None
        assert view.seq_format == 1 and view.qual and not view.lowq
        eng.set_reference(genome5())
        eng.tabulate_view(view)
        eng.sync()
        assert eng.packed_launches() == 1 and eng.libsorts() == 1
        got = eng.finish()
        db.free()
    check(got, *want_grid(70, 20, 3))


# ---------------------------------------------------------------------- 2. a batch made by hand
# name, sequence, where the search for a fitting position starts, CIGAR, flag, reference bases wanted at offsets from pos
# (exact bytes: a lower-case letter asks for the soft-masked stretch), read bases put over the copy of the reference at indices
# of SEQ, qualities (None: absent; "q30": all 30; ("low", i): 30 and a 5 at index i), and the group by construction at
# K = 3 without and with -Q 20.  The read is the reference along the true alignment (insertions and clips 'A') wherever nothing
# is put over it, so only what is written here differs.
N, P5, P3, BOTH = 0, 1, 2, 3
HAND = [
    # an insertion as the first aligned operation: columns 0 and 1 are gaps, the first base behind them is index 2
    ("ins first +", 0, 100, "2I30M", 0, {0: b"C"}, {0: "T", 2: "T"}, "q30", P5, P5),
    ("ins first -", 0, 200, "2I30M", 16, {0: b"C"}, {0: "A", 2: "T"}, "q30", P3, P3),
    # a deletion directly behind the first base: its two columns are positions, the base behind them is index 3
    ("del second +", 0, 300, "1M2D30M", 0, {0: b"C"}, {0: "T"}, "q30", P5, P5),
    ("del second, index 3 +", 0, 400, "1M2D30M", 0, {0: b"A", 3: b"C"}, {1: "T"}, "q30", N, N),
    ("del second -", 0, 500, "1M2D30M", 16, {0: b"C"}, {0: "T"}, "q30", P3, P3),
    # the same at the other end
    ("ins last +", 1, 100, "30M2I", 0, {29: b"G"}, {29: "A", 31: "A"}, "q30", P3, P3),
    ("ins last -", 1, 200, "30M2I", 16, {29: b"G"}, {29: "A"}, "q30", P5, P5),
    ("del before last +", 1, 300, "30M2D1M", 0, {32: b"G"}, {30: "A"}, "q30", P3, P3),
    ("del before last, index 3 +", 1, 400, "30M2D1M", 0, {32: b"A", 29: b"G"}, {29: "A"}, "q30", N, N),
    ("del before last -", 1, 500, "30M2D1M", 16, {32: b"G"}, {30: "A"}, "q30", P5, P5),
    # soft clips are no part of the query; hard clips are ignored
    ("clip, first aligned base", 0, 700, "5S30M", 0, {0: b"C"}, {5: "T"}, "q30", P5, P5),
    ("clip, the pair inside it", 0, 800, "5S30M", 0, {-1: b"C", 0: b"A", 1: b"A", 2: b"A"}, {4: "T"}, "q30", N, N),
    ("hard and soft clips", 0, 900, "3H5S30M4S2H", 0, {0: b"C", 29: b"G"}, {5: "T", 34: "A"}, "q30", BOTH, BOTH),
    # fewer columns than K: both ends see the same columns, and a forward read's C>T is no G>A
    ("one column", 2, 100, "1M", 0, {0: b"C"}, {0: "T"}, "q30", P5, P5),
    ("two columns", 2, 200, "2M", 0, {0: b"A", 1: b"C"}, {1: "T"}, "q30", P5, P5),
    ("two columns, both", 2, 300, "2M", 16, {0: b"C", 1: b"G"}, {0: "T", 1: "A"}, "q30", BOTH, BOTH),
    # index K exactly, and K - 1
    ("index 3", 2, 400, "30M", 0, {3: b"C"}, {3: "T"}, "q30", N, N),
    ("index 2", 2, 500, "30M", 0, {2: b"C"}, {2: "T"}, "q30", P5, P5),
    ("index 3 from the right", 2, 600, "30M", 0, {26: b"G"}, {26: "A"}, "q30", N, N),
    ("index 2 from the right -", 2, 700, "30M", 16, {27: b"G"}, {27: "A"}, "q30", P5, P5),
    # behind an N the two strings are misaligned from the left and aligned from the right (align.py:76-88)
    ("N, last column", 0, 1000, "20M50N10M", 0, {79: b"G"}, {29: "A"}, "q30", P3, P3),
    ("N, the third column pairs with the skipped base", 0, 1200, "2M50N28M", 0, {0: b"A", 1: b"A", 2: b"C", 52: b"T"}, {}, "q30", P5, P5),
    # a read base N, a soft-masked reference stretch
    ("read N", 1, 700, "30M", 0, {0: b"C"}, {0: "N"}, "q30", N, N),
    ("lower-case reference", 0, 6000, "30M", 0, {0: b"c", 29: b"g"}, {0: "T", 29: "A"}, "q30", BOTH, BOTH),
    # the edges of the sequences: chr2 begins TCAGTT, scaf/1:a ends CCGAGG, chr* is the last sequence and ends GTCCCT
    ("position 0", 1, 0, "30M", 0, {0: b"T", 1: b"C"}, {1: "T"}, "q30", P5, P5),
    ("ends at the last base", 3, 2470, "30M", 0, {29: b"G"}, {29: "A"}, "q30", P3, P3),
    ("the last sequence, to its last base", 4, 1970, "30M", 16, {27: b"C", 28: b"C", 29: b"T"}, {}, "q30", N, N),
    ("the last sequence", 4, 100, "30M", 16, {0: b"C"}, {0: "T"}, "q30", P3, P3),
    ("unmapped", -1, -1, "", 4, {}, {}, None, N, N),
    # a terminal T of quality 5 is N / N under -Q 20; without qualities nothing is masked
    ("low quality", 3, 100, "30M", 0, {0: b"C"}, {0: "T"}, ("low", 0), P5, N),
    ("low quality at the other end -", 3, 200, "30M", 16, {0: b"C", 29: b"G"}, {0: "T", 29: "A"}, ("low", 29), BOTH, P3),
    ("no qualities", 3, 300, "30M", 0, {0: b"C"}, {0: "T"}, None, P5, P5),
]
FIXED_POS = {"position 0", "ends at the last base", "the last sequence, to its last base", "unmapped"}


def _fits(contig, pos, ops, wanted):
    span = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
    if pos < 1 or pos + span + 1 > len(contig):
        return False
    if any(contig[pos + off:pos + off + 1] != base for off, base in wanted.items()):
        return False
    # (no base of the window that could pair by accident: only A, C, G, T, in either case)
    return all(chr(c) in "ACGTacgt" for c in contig[pos:pos + span])


def _record(ref, i, name, tid, start, cigar, flag, wanted, put, qual):
    ops = synth._parse_cigar(cigar) if cigar else []
    if tid < 0:
        return dict(flag=flag, lib=i % 2, tid=tid, pos=start, cigar=ops, seq="", qual=None)
    contig = ref.seqs[tid]
    pos = start
    if name in FIXED_POS:
        assert all(contig[pos + off:pos + off + 1] == base for off, base in wanted.items()), name
    else:
        while not _fits(contig, pos, ops, wanted):
            pos += 1
            assert pos < start + 1500, name
    seq, r = [], pos
    for op, ln in ops:
        if op in (0, 7, 8):
            seq.extend(chr(c).upper() for c in contig[r:r + ln])
            r += ln
        elif op in (1, 4):
            seq.extend("A" * ln)
        elif op in (2, 3):
            r += ln
    for at, base in put.items():
        seq[at] = base
    q = None
    if qual is not None:
        q = [30] * len(seq)
        if qual != "q30":
            q[qual[1]] = 5
    return dict(flag=flag, lib=i % 2, tid=tid, pos=pos, cigar=ops, seq="".join(seq), qual=q)


@functools.lru_cache(maxsize=None)
def hand_batch():
    return batch_from_records([_record(genome5(), i, *row[:8]) for i, row in enumerate(HAND)], with_qual=True)


@functools.lru_cache(maxsize=None)
def want_hand(minqual):
    b, libs = hand_batch(), libraries(2)
    group = D.groups_of(D.first_damage(genome5(), b, libs, minqual), 3)
    # the oracle, record by record, confirms every group written down
    assert group.tolist() == [row[9 if minqual else 8] for row in HAND], \
        [(row[0], int(g)) for row, g in zip(HAND, group) if g != row[9 if minqual else 8]]
    groups, kept = yardstick(genome5(), b, libs, group, 4, 70, minqual)
    np.testing.assert_array_equal(kept, brute_kept(b, group, 2, 4))
    return groups, kept, oracle_tableset(genome5(), b, libs, 70, A, minqual)


@pytest.mark.parametrize("minqual", [0, 20])
@pytest.mark.parametrize("form", ["packed", "ascii", "resident"])
def test_hand_made_records(form, minqual):
    with damage_engine(libraries(2), 70, minqual, 3) as eng:
        eng.set_reference(genome5())
        run(eng, hand_batch(), form)
        got = eng.finish()
    check(got, *want_hand(minqual))


# ---------------------------------------------------------------------- 3. more strata than the key kernel counts in the LDS
def test_more_strata_than_the_lds_counts():
    """1 100 libraries x 4 groups = 4 400 strata (csrc/mdx_internal.h LS_LDS_LIBS = 4 096): the kept records are counted
    with global atomics.  (--length 20 and a short length histogram: 4 400 tables come back to the host.)"""
    nl, length, lgd_max = 1100, 20, 512
    b = D.grid_batch().slice(0, 3000)
    group = D.groups_of(D.grid_first(0), 3)[:3000]
    b.lib[:] = (np.arange(3000) * 7 % nl).astype(np.uint16)
    libs = [("S%d" % i, "L") for i in range(nl)]
    want = brute_kept(b, group, nl, 4)
    assert np.count_nonzero(want) > 1500 and all(want.reshape(nl, 4)[:, g].sum() > 0 for g in range(4))
    # (the yardstick's own figures: the kept counts per group of the oracle's runs, every library as one)
    b1 = b.slice(0, b.n)
    b1.lib[:] = 0
    groups, kept1 = yardstick(genome5(), b1, libraries(1), group, 4, length, 0, lgd_max)
    np.testing.assert_array_equal(want.reshape(nl, 4).sum(axis=0), kept1)
    with damage_engine(libs, length, 0, 3, lgd_max=lgd_max) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        got = eng.finish()
    np.testing.assert_array_equal(got.kept, want)
    assert int(got.kept.sum()) == int(((b.flag & 0xF04) == 0).sum()) == got.n_kept
    # the merged block, the libraries summed: the oracle over the untouched batch as one library; every group likewise
    whole = oracle_tableset(genome5(), b1, libraries(1), length, A, 0, lgd_max)
    np.testing.assert_array_equal(got.merged.mis.sum(axis=0), whole.mis[0])
    np.testing.assert_array_equal(got.merged.comp.sum(axis=0), whole.comp[0])
    np.testing.assert_array_equal(got.merged.lgd.sum(axis=0), whole.lgd[0])
    for g in range(4):
        np.testing.assert_array_equal(got.group(g).mis.sum(axis=0), groups[g].mis[0])
        np.testing.assert_array_equal(got.group(g).comp.sum(axis=0), groups[g].comp[0])


# ---------------------------------------------------------------------- 4. accumulation and reset
def test_two_batches_accumulate_and_reset_clears_the_kept_counts():
    b = D.grid_batch()
    with damage_engine(libraries(3), 70, 0, 3) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        assert eng.strata_kept().sum() == 3875
        eng.reset()
        assert not eng.strata_kept().any()
        eng.set_strata_damage(3)                                    # (allowed again: nothing is counted)
        eng.tabulate(b.slice(0, 1501), packed=True)
        eng.tabulate(b.slice(1501, b.n), packed=False)
        check(eng.finish(), *want_grid(70, 0, 3))


# ---------------------------------------------------------------------- 5. errors
def _set(eng, positions, single_stranded=0):
    rc = eng._lib.mdx_set_strata_damage(eng._ctx, positions, single_stranded)
    return rc, eng._lib.mdx_last_error(eng._ctx).decode()


def test_argument_and_state_errors():
    from mapdamage_amd.engine import DamageEngine, MdxError
    b = D.grid_batch().slice(0, 500)
    with DamageEngine(libraries(3), 70, A, 0) as eng:                # three tables: no multiple of the four groups
        rc, msg = _set(eng, 1)
        assert rc == L.MDX_ERR_ARG and "no multiple" in msg
    with DamageEngine(libraries(1), 70, A, 0, groups=D.GROUPS) as eng:
        for positions in (0, -1, 71):
            rc, msg = _set(eng, positions)
            assert rc == L.MDX_ERR_ARG and "positions" in msg, (positions, rc, msg)
        assert eng._lib.mdx_strata_groups(eng._ctx) == 0
        rc, msg = _set(eng, 70, 1)
        assert rc == 0, msg
        assert eng._lib.mdx_strata_groups(eng._ctx) == 4
        # damage strata, then either other kind: one kind per context
        with pytest.raises(MdxError) as err:
            eng.set_strata([0, 1, 2, 3, 0])
        assert err.value.code == L.MDX_ERR_STATE and "mdx_set_strata_damage" in str(err.value)
        with pytest.raises(MdxError) as err:
            eng.set_strata_regions([0, 1, 1, 1, 1, 1], [10], [20], [0])
        assert err.value.code == L.MDX_ERR_STATE and "mdx_set_strata_damage" in str(err.value)
        # the key reads the reference: upload and tabulation before it are refused, with a message that says so
        for packed in (True, False):
            with pytest.raises(MdxError) as err:
                eng.upload(b, packed=packed)
            assert err.value.code == L.MDX_ERR_STATE and "reference" in str(err.value)
        with pytest.raises(MdxError) as err:
            eng.tabulate(b, packed=True)
        assert err.value.code == L.MDX_ERR_STATE and "reference" in str(err.value)
    # ... and this kind after each of the others
    with DamageEngine(libraries(1), 70, A, 0, groups=D.GROUPS) as eng:
        eng.set_strata([0, 1, 2, 3, 0])
        rc, msg = _set(eng, 1)
        assert rc == L.MDX_ERR_STATE and "mdx_set_strata" in msg
    with DamageEngine(libraries(1), 70, A, 0, groups=D.GROUPS) as eng:
        eng.set_strata_regions([0, 1, 1, 1, 1, 1], [10], [20], [0])
        rc, msg = _set(eng, 1)
        assert rc == L.MDX_ERR_STATE and "mdx_set_strata_regions" in msg
    with damage_engine(libraries(3), 70, 0, 1) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        rc, msg = _set(eng, 1)                                       # the setter after a tabulation
        assert rc == L.MDX_ERR_STATE and "counted" in msg
        # the fused tabulate-and-rescale calls count one library
        db = eng.upload(b, packed=False)
        rc = eng._lib.mdx_tabulate_rescale_device(eng._ctx, ctypes.byref(db.dev), None, None, None, None, None)
        assert rc == L.MDX_ERR_ARG and b"mdx_set_strata" in eng._lib.mdx_last_error(eng._ctx)
        db.free()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c", "d"]) as eng:
        with pytest.raises(ValueError, match="groups"):
            eng.set_strata_damage(1)
    with DamageEngine(libraries(1), 70, A, 0) as eng:
        with pytest.raises(ValueError, match="groups"):
            eng.set_strata_damage(1)


# ---------------------------------------------------------------------- 6. the command line
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from mapdamage_amd import fasta, sam
    d = tmp_path_factory.mktemp("damage_cli")
    b, ref = batch4(), genome4()
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg)
    sam.write_sam(str(d / "in.sam"), b, ref.names, ref.lengths, RGS, rg)
    fasta.write_fasta(d / "ref.fa", ref)
    return d


@functools.lru_cache(maxsize=None)
def cli_want(k):
    group = D.groups_of(D.first_damage(genome4(), batch4(), CLI_LIBS, 0), k)
    assert np.bincount(group[(batch4().flag & 0xF04) == 0], minlength=4).min() >= 5
    return yardstick(genome4(), batch4(), CLI_LIBS, group, 4, 70)[0]


def conditional_rows(groups, single_stranded=False):
    """``conditional.tsv`` from the yardstick's tables of the four groups, with plain numpy sums."""
    ct, c, ga, g = (L.MIS_COLS.index(x) for x in ("C>T", "C", "G>A", "G"))
    e3, e5 = L.ENDS.index("3p"), L.ENDS.index("5p")
    rows = ["Sample\tLibrary\tEnd\tPos\tGiven\tSubstitutions\tBases\tFrequency"]
    for (sample, library), li in sorted((lib, i) for i, lib in enumerate(CLI_LIBS)):
        for end, ei, num, den, given in (("5p", e5, ct, c, (("all", (0, 1, 2, 3)), ("3p-damaged", (2, 3)), ("3p-undamaged", (0, 1)))),
                                         ("3p", e3) + ((ct, c) if single_stranded else (ga, g)) +
                                         ((("all", (0, 1, 2, 3)), ("5p-damaged", (1, 3)), ("5p-undamaged", (0, 2))),)):
            for name, members in given:
                mis = np.sum([groups[m].mis[li, ei] for m in members], axis=(0, 1))          # [pos][col], strands summed
                for p in range(70):
                    s, b = int(mis[p, num]), int(mis[p, den])
                    rows.append("%s\t%s\t%s\t%d\t%s\t%d\t%d\t%s" % (sample, library, end, p + 1, name, s, b, "%.15g" % (s / b) if b else "NaN"))
    return "\n".join(rows) + "\n"


def check_tree(out, k):
    groups = cli_want(k)
    files = tree(out / "by_damage")
    assert sorted(files) == sorted(["groups.tsv", "conditional.tsv"] + ["%d/%s" % (g, f) for g in range(4) for f in FILES])
    assert files["groups.tsv"] == "Index\tGroup\tReads\n" + "".join("%d\t%s\t%d\n" % (g, D.GROUPS[g], groups[g].n_kept) for g in range(4))
    for g, t in enumerate(groups):
        assert files["%d/misincorporation.txt" % g] == t.misincorporation_text()
        assert files["%d/dnacomp.txt" % g] == t.dnacomp_text()
        assert files["%d/lgdistribution.txt" % g] == t.lgdistribution_text()
    assert files["conditional.tsv"] == conditional_rows(groups)


def run_cli(d, out, *args):
    from mapdamage_amd.main import main
    assert main(["-r", str(d / "ref.fa"), "-d", str(out), "--no-stats"] + [str(a) for a in args]) == 0
    return out


def test_command_line_three_routes(cli_files, tmp_path):
    d = cli_files
    plain = run_cli(d, tmp_path / "plain", "-i", d / "in.bam")
    assert not (plain / "by_damage").exists()
    extra = ["--by-terminal-damage", "--terminal-positions", "2"]
    outs = [run_cli(d, tmp_path / "bam", "-i", d / "in.bam", *extra),
            run_cli(d, tmp_path / "host", "-i", d / "in.bam", "--host-decode", *extra),
            run_cli(d, tmp_path / "sam", "-i", d / "in.sam", *extra)]
    assert "GPU decode path gave up" not in (outs[0] / "Runtime_log.txt").read_text()
    first = tree(outs[0] / "by_damage")
    for o in outs[1:]:
        assert tree(o / "by_damage") == first
    check_tree(outs[0], 2)
    for o in outs:
        assert not (o / "by_reference").exists() and not (o / "by_region").exists()
        for f in FILES:
            assert (o / f).read_text() == (plain / f).read_text(), (o, f)
    # the default is one position
    check_tree(run_cli(d, tmp_path / "one", "-i", d / "in.bam", "--by-terminal-damage"), 1)


def test_two_ranks_write_the_same_tree(cli_files, tmp_path):
    """``--gpus 2`` in a process of its own (one that has not touched the GPU before the run does), against the yardstick."""
    d = cli_files
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    # (several slabs out of a small file: both ranks decode and count)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1", MDX_GBAM_SLAB_BYTES="65536")
    cmd = [sys.executable, "-m", "mapdamage_amd", "-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / "two"),
           "--no-stats", "--by-terminal-damage", "--terminal-positions", "2", "--gpus", "2", "--share-gpu", "--dist-backend", "gloo"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    check_tree(tmp_path / "two", 2)
    want = oracle_tableset(genome4(), batch4(), CLI_LIBS, 70, A, 0)
    assert (tmp_path / "two" / "misincorporation.txt").read_text() == want.misincorporation_text()
    assert (tmp_path / "two" / "dnacomp.txt").read_text() == want.dnacomp_text()
    assert (tmp_path / "two" / "lgdistribution.txt").read_text() == want.lgdistribution_text()


# ---------------------------------------------------------------------- 7. --stats
def test_stats_by_terminal_damage(tmp_path):
    """Every group with data gets a chain of its own: its three CSV files equal those of a run over that group's records
    alone (tests/test_gpu_stats.py ``test_stats_by_reference``)."""
    from mapdamage_amd import fasta, sam, stats
    from mapdamage_amd.main import main
    from tests.test_gpu_stats import CSVS, FAST
    rgs = [{"ID": "rg1", "SM": "s1", "LB": "lib1"}]
    ref = synth.make_genome(seed=61, sizes=(("chrA", 6000), ("chrB", 4000), ("chrC", 3000)), n_run=40, lower_run=200)
    batch = synth.make_reads(ref, 6000, 62, read_len=60, with_qual=True)
    group = D.groups_of(D.first_damage(ref, batch, [("s1", "lib1")], 0), 1)
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    sam.write_bam(str(tmp_path / "in.bam"), batch, ref.names, ref.lengths, rgs, ["rg1"] * batch.n)
    out = tmp_path / "out"
    assert main(["-i", str(tmp_path / "in.bam"), "-r", str(tmp_path / "ref.fa"), "-d", str(out), "--stats", "--by-terminal-damage"] + FAST) == 0
    with_data = 0
    for g in range(4):
        part = batch.take(np.flatnonzero(group == g))
        mis = oracle_tableset(ref, part, [("s1", "lib1")], 70, A, 0).mis
        has_data = bool(mis[:, L.ENDS.index("5p"), :, 0, L.MIS_COLS.index("C")].sum()) and \
            bool(mis[:, L.ENDS.index("3p"), :, 0, L.MIS_COLS.index("G")].sum())
        if not has_data:
            assert not any((out / "by_damage" / str(g) / name).exists() for name in CSVS)
            continue
        with_data += 1
        sam.write_bam(str(tmp_path / ("only%d.bam" % g)), part, ref.names, ref.lengths, rgs, ["rg1"] * part.n)
        alone = tmp_path / ("alone%d" % g)
        assert main(["-i", str(tmp_path / ("only%d.bam" % g)), "-r", str(tmp_path / "ref.fa"), "-d", str(alone), "--stats",
                     "--stats-chain", str(g + 1)] + FAST) == 0
        for name in CSVS:
            assert (out / "by_damage" / str(g) / name).read_bytes() == (alone / name).read_bytes(), (g, name)
    assert with_data >= 3
    assert (out / stats.CORR_CSV).read_bytes() != (out / "by_damage" / "0" / stats.CORR_CSV).read_bytes()
