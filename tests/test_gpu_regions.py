"""Region strata on the device: tables per (library, group of genomic regions) from one pass (include/mdx.h
``mdx_set_strata_regions``; ``--regions`` / ``--region-groups``).

The yardstick follows tests/test_gpu_strata.py: for a stratum, the oracle over the same batch with FLAG 0x4 set on every
record outside it.  Tables bit for bit, texts byte for byte, the merged block equal to the oracle over the untouched batch.
A record's group comes from tests/regions_util.py — every record against every region of its sequence, in numpy — which
shares nothing with the product: the product assigns on the device only."""

import ctypes
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import synth
from mapdamage_amd.batch import batch_from_records, concat_batches
from mapdamage_amd.tables import TableSet
from tests import regions_util as R
from tests.test_gpu_strata import A, FILES, MIXED, batch4, batch5, check, genome4, genome5, libraries, tree
from tests.util import oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def columns(regions, n_contig):
    """(iv_off, iv_start, iv_end, iv_group) of a list of disjoint ``(tid, start, end, group)``."""
    r = np.asarray(sorted(regions), np.int64).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum(np.bincount(r[:, 0], minlength=n_contig))]).astype(np.int64)
    return off, r[:, 1].astype(np.int32), r[:, 2].astype(np.int32), r[:, 3].astype(np.int32)


def yardstick(ref, batch, libs, group, n_groups, length, minqual=0, lgd_max=65536):
    """(per-group TableSets over the libraries, kept reads per stratum) for the per-record ``group``: one oracle run per
    stratum, every record outside it flagged unmapped (tests/test_gpu_strata.py ``yardstick``)."""
    nl = len(libs)
    kept = np.zeros(nl * n_groups, np.uint64)
    out = []
    for g in range(n_groups):
        parts = []
        for li in range(nl):
            flag = batch.flag.copy()
            flag[~((group == g) & (batch.lib == li))] |= 0x4
            t = oracle_tableset(ref, dataclasses.replace(batch, flag=flag), libs, length, A, minqual, lgd_max)
            others = [x for x in range(nl) if x != li]
            assert not t.mis[others].any() and not t.comp[others].any() and not t.lgd[others].any()
            kept[li * n_groups + g] = t.n_kept
            parts.append(t)
        out.append(TableSet(list(libs), length, A, np.stack([parts[li].mis[li] for li in range(nl)]),
                            np.stack([parts[li].comp[li] for li in range(nl)]), np.stack([parts[li].lgd[li] for li in range(nl)]),
                            np.concatenate([p.lgd_over.reshape(-1, 4) for p in parts]), sum(p.n_kept for p in parts)))
    return out, kept


def brute_kept(batch, group, n_libraries, n_groups):
    keep = (batch.flag & 0xF04) == 0
    return np.bincount(batch.lib[keep].astype(np.int64) * n_groups + group[keep], minlength=n_libraries * n_groups).astype(np.uint64)


def run(eng, b, form):
    if form == "resident":
        db = eng.upload(b, packed=True)
        eng.tabulate(db)
        eng.sync()
        assert eng.libsorts() == 0
        db.free()
    else:
        eng.tabulate(b, packed=form == "packed")


# ---------------------------------------------------------------------- 1. the grid
@functools.lru_cache(maxsize=None)
def grid_group():
    b, regs = batch5(), R.grid_regions()
    assert 35 <= len(regs) <= 45 and {g for _, _, _, g in regs} == {0, 1, 2}
    assert not any(t == 2 for t, _, _, _ in regs) and all(1 <= e - s <= 900 for _, s, e, _ in regs)
    assert sorted((s, e) for t, s, e, _ in regs if t == 4)[0][0] == 0 and sum(e - s for t, s, e, _ in regs if t == 4) == 2000
    found = R.edge_classes(b, regs, 5, 3)
    for name in R.CLASSES:
        assert len(found[name]) >= 1, name
    return R.brute_group(b, regs, 5, 3)


@functools.lru_cache(maxsize=None)
def want_grid(length, minqual):
    libs = libraries(3)
    groups, kept = yardstick(genome5(), batch5(), libs, grid_group(), 4, length, minqual)
    np.testing.assert_array_equal(kept, brute_kept(batch5(), grid_group(), 3, 4))
    return groups, kept, oracle_tableset(genome5(), batch5(), libs, length, A, minqual)


@pytest.mark.parametrize("form", ["packed", "ascii", "resident"])
@pytest.mark.parametrize("length,minqual", [(70, 0), (70, 20), (700, 0), (700, 20)])
def test_grid(length, minqual, form):
    from mapdamage_amd.engine import DamageEngine
    b = batch5()
    with DamageEngine(libraries(3), length, A, minqual, groups=R.GRID_GROUPS) as eng:
        assert eng.table_mode == ("global" if length == 700 else "lds")
        eng.set_strata_regions(*columns(R.grid_regions(), 5))
        eng.set_reference(genome5())
        lib_before = b.lib.copy()
        run(eng, b, form)
        if length == 70:
            assert eng.packed_launches() == (0 if form == "ascii" else 1)
        got = eng.finish()
        np.testing.assert_array_equal(b.lib, lib_before)
    check(got, *want_grid(length, minqual))


# ---------------------------------------------------------------------- 2. a boundary batch made by hand
HAND_REGIONS = [(0, 0, 1, 0), (0, 100, 200, 0), (0, 200, 300, 1), (0, 500, 501, 1), (0, 8990, 9000, 0), (1, 1000, 1100, 1)]
# (sequence, pos, CIGAR, flag, the group the rule gives — 2 is '*'), one per class of tests/regions_util.py CLASSES and more
HAND = [(0, 60, "40M", 0, 2),              # [60, 100): ends exactly at a region's start
        (0, 300, "30M", 16, 2),            # starts exactly at a region's end
        (0, 61, "40M", 0, 0),              # one base on the left
        (0, 299, "30M", 0, 1),             # one base on the right
        (0, 480, "50M", 16, 1),            # contains a whole region
        (0, 180, "40M", 0, 0),             # two groups: the one that begins first
        (0, 200, "40M", 0, 1),             # ... from its first base
        (1, 960, "30M15D5M", 0, 1),        # [960, 1010): the aligned bases alone end at 995
        (1, 900, "20M81N5M", 16, 1),       # [900, 1006) through an N
        (1, 1100, "10S30M", 0, 2),         # the clip would reach back into [1000, 1100)
        (1, 970, "30M10S", 0, 2),          # [970, 1000): the clip would reach forward
        (1, 968, "2H30M10S3H", 0, 2),      # [968, 998)
        (2, 100, "30M", 0, 2),             # a sequence without regions
        (-1, -1, "", 4, 2),                # no sequence (unmapped: the flag filter drops it)
        (0, 500, "6I", 0, 1),              # no reference-consuming op: [500, 501), on a one-base region
        (0, 501, "12S", 0, 2),             # ... and beside it
        (0, 499, "3S4I2S", 16, 2),
        (0, 0, "25M", 0, 0),               # the first interval of a sequence
        (0, 1, "25M", 0, 2),
        (0, 8960, "31M", 0, 0),            # the last: [8960, 8991)
        (0, 8960, "30M", 16, 2),
        (1, 1099, "20M", 0, 1),            # the last of another sequence
        (1, 3000, "20M", 0, 2),            # behind it
        (4, 10, "20M", 0, 2)]              # the last sequence, no regions


@functools.lru_cache(maxsize=None)
def hand_batch():
    rng = np.random.default_rng(3)
    recs = []
    for i, (tid, pos, cigar, flag, _) in enumerate(HAND):
        ops = synth._parse_cigar(cigar)
        n = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        recs.append(dict(flag=flag, lib=i % 2, tid=tid, pos=pos, cigar=ops, seq="".join("ACGT"[k] for k in rng.integers(0, 4, n))))
    return batch_from_records(recs, with_qual=False)


@pytest.mark.parametrize("form", ["packed", "ascii", "resident"])
def test_hand_made_boundaries(form):
    from mapdamage_amd.engine import DamageEngine
    b, libs = hand_batch(), libraries(2)
    group = R.brute_group(b, HAND_REGIONS, 5, 2)
    assert group.tolist() == [g for *_, g in HAND]                 # (the brute force agrees with the rule read by hand)
    found = R.edge_classes(b, HAND_REGIONS, 5, 2)
    assert all(found[name] for name in R.CLASSES)
    want_groups, want_kept = yardstick(genome5(), b, libs, group, 3, 70)
    np.testing.assert_array_equal(want_kept, brute_kept(b, group, 2, 3))
    with DamageEngine(libs, 70, A, 0, groups=["a", "b", "*"]) as eng:
        eng.set_strata_regions(*columns(HAND_REGIONS, 5))
        eng.set_reference(genome5())
        run(eng, b, form)
        got = eng.finish()
    check(got, want_groups, want_kept, oracle_tableset(genome5(), b, libs, 70, A, 0))


# ---------------------------------------------------------------------- 3. a deep search
def test_deep_search():
    """5 000 one-base regions on every other base, two alternating groups: the slice's binary search takes 13 steps."""
    from mapdamage_amd.engine import DamageEngine
    ref = synth.make_genome(seed=61, sizes=(("deep", 12000),), n_run=40, lower_run=200)
    regs = [(0, 2 * k, 2 * k + 1, k % 2) for k in range(5000)]
    mixed = synth.make_reads(ref, 8000, 62, len_range=(20, 60), **{k: v for k, v in MIXED.items() if k != "len_range"})
    # (a read of two bases and more always meets a region below base 9 999: one-base reads fall between them as well)
    ones = batch_from_records([dict(flag=16 * (p % 3 == 0), tid=0, pos=p, cigar=[(0, 1)], seq="A") for p in range(4000, 4200)] +
                              [dict(flag=0, tid=0, pos=p, cigar=[(0, 1)], seq="C") for p in range(9990, 10010)], with_qual=False)
    b = concat_batches([mixed, ones])
    group = R.brute_group(b, regs, 1, 2)
    keep = (b.flag & 0xF04) == 0
    assert all(np.count_nonzero(keep & (group == g)) > 100 for g in range(3))
    assert (group[mixed.n:mixed.n + 200] == np.where(np.arange(4000, 4200) % 2 == 1, 2, (np.arange(4000, 4200) // 2) % 2)).all()
    libs = libraries(1)
    want_groups, want_kept = yardstick(ref, b, libs, group, 3, 70)
    with DamageEngine(libs, 70, A, 0, groups=["even", "odd", "*"]) as eng:
        eng.set_strata_regions(*columns(regs, 1))
        eng.set_reference(ref)
        eng.tabulate(b, packed=True)
        got = eng.finish()
    check(got, want_groups, want_kept, oracle_tableset(ref, b, libs, 70, A, 0))


# ---------------------------------------------------------------------- 4. more strata than the key kernel counts in the LDS
def test_more_strata_than_the_lds_counts():
    """2 libraries x 2 100 groups = 4 200 strata (csrc/mdx_internal.h LS_LDS_LIBS = 4 096): the kept records are counted
    with global atomics."""
    from mapdamage_amd.engine import DamageEngine
    ng = 2100
    regs = [(0, 4 * k, 4 * k + 2, k % (ng - 1)) for k in range(2200)] + [(1, 7 * k, 7 * k + 1, (5 * k) % (ng - 1)) for k in range(700)]
    b = batch5().slice(0, 3000)
    b.lib[:] = b.lib % 2
    group = R.brute_group(b, regs, 5, ng - 1)
    want = brute_kept(b, group, 2, ng)
    assert np.count_nonzero(want) > 500 and want[ng - 1] > 0 and want[2 * ng - 1] > 0
    with DamageEngine(libraries(2), 70, A, 0, lgd_max=1024, groups=["g%d" % i for i in range(ng - 1)] + ["*"]) as eng:
        eng.set_strata_regions(*columns(regs, 5))
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        eng.sync()
        kept = eng.strata_kept()
    assert int(kept.sum()) == int(((b.flag & 0xF04) == 0).sum())
    np.testing.assert_array_equal(kept, want)


# ---------------------------------------------------------------------- 5. accumulation and reset
def test_two_batches_accumulate_and_reset_clears_the_kept_counts():
    from mapdamage_amd.engine import DamageEngine
    b = batch5()
    with DamageEngine(libraries(3), 70, A, 0, groups=R.GRID_GROUPS) as eng:
        eng.set_strata_regions(*columns(R.grid_regions(), 5))
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        eng.reset()
        assert not eng.strata_kept().any()
        eng.set_strata_regions(*columns(R.grid_regions(), 5))       # (allowed again: nothing is counted)
        eng.tabulate(b.slice(0, 7001), packed=True)
        eng.tabulate(b.slice(7001, b.n), packed=False)
        check(eng.finish(), *want_grid(70, 0))


# ---------------------------------------------------------------------- 6. errors
def _set(eng, n_groups, n_contig, off, start, end, group, rest):
    arrays = [np.ascontiguousarray(off, np.int64)] + [np.ascontiguousarray(a, np.int32) for a in (start, end, group)]
    rc = eng._lib.mdx_set_strata_regions(eng._ctx, n_groups, n_contig, *[ctypes.c_void_p(a.ctypes.data) for a in arrays], rest)
    return rc, eng._lib.mdx_last_error(eng._ctx).decode()


def test_argument_and_state_errors():
    from mapdamage_amd.engine import DamageEngine, MdxError
    from mapdamage_amd import layout as L
    good = ([0, 2, 3], [10, 30, 5], [20, 40, 6], [0, 1, 0])
    with DamageEngine(libraries(3), 70, A, 0) as eng:                # three tables, two groups
        rc, msg = _set(eng, 2, 2, *good, 1)
        assert rc == L.MDX_ERR_ARG and "no multiple" in msg
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b"]) as eng:
        for off, start, end, group, rest, words in [
                ([0, 2, 3], [30, 10, 5], [40, 20, 6], [0, 1, 0], 1, ["interval 1", "sorted"]),           # unsorted
                ([0, 2, 3], [10, 19, 5], [20, 40, 6], [0, 1, 0], 1, ["interval 1", "interval 0"]),       # overlapping
                ([0, 1, 3], [10, 30, 30], [20, 40, 41], [0, 1, 0], 1, ["interval 2", "sequence 1"]),     # ... in the second sequence
                ([0, 2, 3], [10, 30, 5], [20, 40, 6], [0, 1, 2], 1, ["interval 2", "group 2"]),          # a group out of range
                ([0, 2, 3], [10, 30, 5], [20, 40, 6], [0, -1, 0], 1, ["interval 1", "group -1"]),
                ([0, 2, 3], [10, 30, 5], [20, 30, 6], [0, 1, 0], 1, ["interval 1", "start < end"]),      # empty
                ([0, 2, 3], [-1, 30, 5], [20, 40, 6], [0, 1, 0], 1, ["interval 0", "start < end"]),
                ([0, 2, 1], [10, 30, 5], [20, 40, 6], [0, 1, 0], 1, ["offsets", "sequence 1"]),          # offsets not monotone
                ([0, 2, 3], [10, 30, 5], [20, 40, 6], [0, 1, 0], 2, ["rest_group"])]:
            rc, msg = _set(eng, 2, 2, off, start, end, group, rest)
            assert rc == L.MDX_ERR_ARG and all(w in msg for w in words), (rc, msg)
        assert eng._lib.mdx_strata_groups(eng._ctx) == 0
        # abutting intervals are disjoint
        rc, msg = _set(eng, 2, 2, [0, 2, 3], [10, 20, 5], [20, 40, 6], [0, 1, 0], 1)
        assert rc == 0, msg
        assert eng._lib.mdx_strata_groups(eng._ctx) == 2
        # region strata, then tid strata: one kind per context
        with pytest.raises(MdxError) as err:
            eng.set_strata([0, 1])
        assert err.value.code == L.MDX_ERR_STATE
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b"]) as eng:
        eng.set_strata([0, 1, 0, 1, 0])
        rc, msg = _set(eng, 2, 2, *good, 1)
        assert rc == L.MDX_ERR_STATE and "mdx_set_strata" in msg
    with DamageEngine(libraries(3), 70, A, 0, groups=R.GRID_GROUPS) as eng:
        cols = columns(R.grid_regions(), 5)
        eng.set_strata_regions(*cols)
        eng.set_reference(genome5())
        eng.tabulate(batch5().slice(0, 500), packed=True)
        with pytest.raises(MdxError) as err:
            eng.set_strata_regions(*cols)
        assert err.value.code == L.MDX_ERR_STATE
        # the fused tabulate-and-rescale calls count one library
        db = eng.upload(batch5().slice(0, 500), packed=False)
        rc = eng._lib.mdx_tabulate_rescale_device(eng._ctx, ctypes.byref(db.dev), None, None, None, None, None)
        assert rc == L.MDX_ERR_ARG and b"mdx_set_strata" in eng._lib.mdx_last_error(eng._ctx)
        db.free()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b"]) as eng:
        eng.set_strata_regions(*good)                               # two sequences, the reference has five
        eng.set_reference(genome5())
        with pytest.raises(MdxError) as err:
            eng.tabulate(batch5().slice(0, 500), packed=True)
        assert err.value.code == L.MDX_ERR_ARG and "mdx_set_strata_regions named 2" in str(err.value)
    with DamageEngine(libraries(1), 70, A, 0) as eng:
        with pytest.raises(ValueError, match="without groups"):
            eng.set_strata_regions(*good)


# ---------------------------------------------------------------------- 7. the command line
RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s1", "LB": "lib2"}]
CLI_LIBS = [("s1", "lib1"), ("s1", "lib2")]
CLI_NAMES = ["tgt a", "x:y", "third", "*"]
# (as the BED lists them: unsorted, the first three merge into [100, 700), groups numbered by first appearance)
CLI_REGIONS = [(0, 400, 450, 0), (3, 500, 1500, 1), (0, 100, 400, 0), (0, 430, 700, 0), (0, 1000, 1001, 1), (0, 1001, 1900, 2),
               (1, 2000, 2600, 0), (0, 5000, 5900, 1), (1, 50, 60, 2), (3, 1500, 1530, 2)]


@functools.lru_cache(maxsize=None)
def cli_group():
    return R.brute_group(batch4(), CLI_REGIONS, 4, 3)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from mapdamage_amd import fasta, sam
    d = tmp_path_factory.mktemp("regions_cli")
    b, ref = batch4(), genome4()
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg)
    sam.write_sam(str(d / "in.sam"), b, ref.names, ref.lengths, RGS, rg)
    fasta.write_fasta(d / "ref.fa", ref)
    (d / "groups.bed").write_text("track name=panel\n# a comment\n" + R.bed_text(CLI_REGIONS, ref.names, CLI_NAMES))
    (d / "plain.bed").write_text(R.bed_text(CLI_REGIONS, ref.names))
    return d


def run_cli(d, out, *args):
    from mapdamage_amd.main import main
    assert main(["-r", str(d / "ref.fa"), "-d", str(out), "--no-stats"] + [str(a) for a in args]) == 0
    return out


def check_tree(out, names, group, regions):
    ng = len(names)
    groups, _ = yardstick(genome4(), batch4(), CLI_LIBS, group, ng, 70)
    files = tree(out / "by_region")
    assert sorted(files) == sorted(["groups.tsv"] + ["%d/%s" % (g, f) for g in range(ng) for f in FILES])
    n_regions, n_bases = R.merged_figures(regions, genome4().lengths, ng)
    assert files["groups.tsv"] == "Index\tGroup\tRegions\tBases\tReads\n" + "".join(
        "%d\t%s\t%d\t%d\t%d\n" % (g, names[g], n_regions[g], n_bases[g], groups[g].n_kept) for g in range(ng))
    for g, t in enumerate(groups):
        assert files["%d/misincorporation.txt" % g] == t.misincorporation_text()
        assert files["%d/dnacomp.txt" % g] == t.dnacomp_text()
        assert files["%d/lgdistribution.txt" % g] == t.lgdistribution_text()


def test_command_line_three_routes(cli_files, tmp_path):
    d = cli_files
    plain = run_cli(d, tmp_path / "plain", "-i", d / "in.bam")
    assert not (plain / "by_region").exists()
    outs = [run_cli(d, tmp_path / "bam", "-i", d / "in.bam", "--region-groups", d / "groups.bed"),
            run_cli(d, tmp_path / "host", "-i", d / "in.bam", "--region-groups", d / "groups.bed", "--host-decode"),
            run_cli(d, tmp_path / "sam", "-i", d / "in.sam", "--region-groups", d / "groups.bed")]
    assert "GPU decode path gave up" not in (outs[0] / "Runtime_log.txt").read_text()
    first = tree(outs[0] / "by_region")
    for o in outs[1:]:
        assert tree(o / "by_region") == first
    assert np.bincount(cli_group(), minlength=4).min() > 50
    check_tree(outs[0], CLI_NAMES, cli_group(), CLI_REGIONS)
    for o in outs:
        assert not (o / "by_reference").exists()
        for f in FILES:
            assert (o / f).read_text() == (plain / f).read_text(), (o, f)
    # a region beyond its sequence: an error that names the line, no tables
    (tmp_path / "bad.bed").write_text("chrM\t0\t10\ta\nchrM\t2400\t2501\tb\n")
    from mapdamage_amd.main import main
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / "bad"), "--region-groups",
                 str(tmp_path / "bad.bed")]) == 1
    assert "line 2" in (tmp_path / "bad" / "Runtime_log.txt").read_text()
    assert not (tmp_path / "bad" / "misincorporation.txt").exists()


def test_only_regions_is_the_filtered_run(cli_files, tmp_path):
    d = cli_files
    out = run_cli(d, tmp_path / "only", "-i", d / "in.bam", "--regions", d / "plain.bed", "--only-regions")
    b = batch4()
    inside = np.where(cli_group() == 3, 1, 0)                        # one group 'regions' (0), then '*' (1)
    flag = b.flag.copy()
    flag[inside == 1] |= 0x4
    want = oracle_tableset(genome4(), dataclasses.replace(b, flag=flag), CLI_LIBS, 70, A, 0)
    assert 0 < want.n_kept < int(((b.flag & 0xF04) == 0).sum())
    assert (out / "misincorporation.txt").read_text() == want.misincorporation_text()
    assert (out / "dnacomp.txt").read_text() == want.dnacomp_text()
    assert (out / "lgdistribution.txt").read_text() == want.lgdistribution_text()
    # by_region/ is complete, '*' included
    check_tree(out, ["regions", "*"], inside, [(t, s, e, 0) for t, s, e, _ in CLI_REGIONS])


def test_two_ranks_write_the_same_tree(cli_files, tmp_path):
    """``--gpus 2`` in a process of its own (one that has not touched the GPU before the run does), against the yardstick."""
    d = cli_files
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    # (several slabs out of a small file: both ranks decode and count)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1", MDX_GBAM_SLAB_BYTES="65536")
    cmd = [sys.executable, "-m", "mapdamage_amd", "-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / "two"),
           "--no-stats", "--region-groups", str(d / "groups.bed"), "--gpus", "2", "--share-gpu", "--dist-backend", "gloo"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    check_tree(tmp_path / "two", CLI_NAMES, cli_group(), CLI_REGIONS)
    want = oracle_tableset(genome4(), batch4(), CLI_LIBS, 70, A, 0)
    assert (tmp_path / "two" / "misincorporation.txt").read_text() == want.misincorporation_text()
    assert (tmp_path / "two" / "dnacomp.txt").read_text() == want.dnacomp_text()
    assert (tmp_path / "two" / "lgdistribution.txt").read_text() == want.lgdistribution_text()
