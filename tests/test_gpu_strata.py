"""Strata on the device: tables per (library, group of reference sequences) from one pass (include/mdx.h ``mdx_set_strata``).

The yardstick for a stratum is the oracle over the same batch with FLAG 0x4 set on every record that is not in that stratum:
the reference's filter (reader.py:121-132) drops those records, what is left is the stratum.  Tables bit for bit, text files
byte for byte with what the emitters write for the oracle's tables of that subset; the merged block equals the oracle over
the untouched batch and the sum of the strata."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import synth
from mapdamage_amd.tables import TableSet
from tests.util import assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 10
FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")
MIXED = dict(len_range=(20, 130), frac_softclip=0.15, frac_ins=0.08, frac_del=0.08, frac_skip=0.02, frac_hardclip=0.005,
             frac_filtered=0.03, frac_n_base=0.02)


def libraries(n):
    return [("S%d" % i, "L%d" % i) for i in range(n)]


def yardstick(ref, batch, libs, group_of_tid, n_groups, length, minqual=0, lgd_max=65536):
    """(per-group TableSets over the libraries, kept reads per stratum): one oracle run per stratum, every record outside
    it flagged unmapped; the run's table of the stratum's library is the stratum — its other tables stay empty."""
    import dataclasses
    group = np.asarray(group_of_tid)[np.clip(batch.tid, 0, len(group_of_tid) - 1)]
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
            assert all(int(row[0]) == li for row in t.lgd_over)
            kept[li * n_groups + g] = t.n_kept
            parts.append(t)
        mis = np.stack([parts[li].mis[li] for li in range(nl)])
        comp = np.stack([parts[li].comp[li] for li in range(nl)])
        lgd = np.stack([parts[li].lgd[li] for li in range(nl)])
        over = np.concatenate([p.lgd_over.reshape(-1, 4) for p in parts])
        out.append(TableSet(list(libs), length, A, mis, comp, lgd, over, sum(p.n_kept for p in parts)))
    return out, kept


def check(got, want_groups, want_kept, want_all):
    """A ``StratifiedTables`` against the yardstick: every stratum, the merged block, their sum, the texts."""
    np.testing.assert_array_equal(got.kept, want_kept)
    total = None
    for g, want in enumerate(want_groups):
        t = got.group(g)
        assert_tables_equal(t, want)
        assert t.misincorporation_text() == want.misincorporation_text()
        assert t.dnacomp_text() == want.dnacomp_text()
        assert t.lgdistribution_text() == want.lgdistribution_text()
        total = t if total is None else total.add(t)
    assert_tables_equal(got.merged, want_all)
    assert_tables_equal(total, got.merged)
    assert got.merged.misincorporation_text() == want_all.misincorporation_text()


# ---------------------------------------------------------------------- 1. the basic grid
GROUP_OF_TID = [0, 1, 0, 2, 1]


@functools.lru_cache(maxsize=None)
def genome5():
    return synth.make_genome(seed=23, sizes=(("chr1", 9000), ("chr2", 5000), ("chrM", 3000), ("scaf/1:a", 2500), ("chr*", 2000)),
                             n_run=40, lower_run=200)


@functools.lru_cache(maxsize=None)
def batch5():
    b = synth.make_reads(genome5(), 20_000, 77, nlib=3, with_qual=True, **MIXED)
    rng = np.random.default_rng(78)
    nb = b.seq.shape[0]
    b.qual = np.where(rng.random(nb) < 0.05, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    assert set(np.unique(b.tid)) == {0, 1, 2, 3, 4} and (b.flag & 0x10).any() and not (b.flag & 0x10).all()
    return b


@functools.lru_cache(maxsize=None)
def want5(length, minqual):
    libs = libraries(3)
    groups, kept = yardstick(genome5(), batch5(), libs, GROUP_OF_TID, 3, length, minqual)
    return groups, kept, oracle_tableset(genome5(), batch5(), libs, length, A, minqual)


@pytest.mark.parametrize("length,minqual,form", [(70, 0, "packed"), (70, 20, "packed"), (700, 0, "packed"), (70, 0, "ascii"),
                                                 (70, 20, "ascii"), (70, 0, "resident"), (70, 20, "resident")])
def test_basic_grid(length, minqual, form):
    from mapdamage_amd.engine import DamageEngine
    b = batch5()
    with DamageEngine(libraries(3), length, A, minqual, groups=["g0", "g1", "g2"]) as eng:
        assert eng.table_mode == ("global" if length == 700 else "lds")
        eng.set_strata(GROUP_OF_TID)
        eng.set_reference(genome5())
        lib_before = b.lib.copy()
        if form == "resident":
            # (a resident batch brings its columns bucketed by stratum: no key column is made per launch)
            db = eng.upload(b, packed=True)
            eng.tabulate(db)
            eng.sync()
            assert eng.libsorts() == 0
            db.free()
        else:
            eng.tabulate(b, packed=form == "packed")
        if length == 70:
            assert eng.packed_launches() == (0 if form == "ascii" else 1)
        got = eng.finish()
        np.testing.assert_array_equal(b.lib, lib_before)
    check(got, *want5(length, minqual))


def test_two_batches_accumulate_and_reset_clears_the_kept_counts():
    from mapdamage_amd.engine import DamageEngine
    b = batch5()
    with DamageEngine(libraries(3), 70, A, 0, groups=["g0", "g1", "g2"]) as eng:
        eng.set_strata(GROUP_OF_TID)
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        eng.reset()
        assert not eng.strata_kept().any()
        eng.set_strata(GROUP_OF_TID)            # (allowed again: nothing is counted)
        eng.tabulate(b.slice(0, 7001), packed=True)
        eng.tabulate(b.slice(7001, b.n), packed=False)
        check(eng.finish(), *want5(70, 0))


# ---------------------------------------------------------------------- 2, 3. more strata than a launch takes
N130 = 130
EMPTY = list(range(3, 130, 13))              # ten sequences without a read
DROPPED = [5, 31, 64, 97, 128]               # five whose reads the flag filter drops, all of them


@functools.lru_cache(maxsize=None)
def genome130():
    return synth.make_genome(seed=31, sizes=tuple(("contig_%d" % i, 2000) for i in range(N130)), n_run=40, lower_run=200)


@functools.lru_cache(maxsize=None)
def batch130():
    assert len(EMPTY) == 10 and not set(EMPTY) & set(DROPPED)
    b = synth.make_reads(genome130(), 30_000, 91, contigs=[i for i in range(N130) if i not in EMPTY], **MIXED)
    b.flag[np.isin(b.tid, DROPPED)] |= 0x400
    return b


@functools.lru_cache(maxsize=None)
def want130():
    libs = libraries(1)
    groups, kept = yardstick(genome130(), batch130(), libs, list(range(N130)), N130, 70, 0, 1024)
    assert sum(1 for k in kept if k == 0) == 15
    return groups, kept, oracle_tableset(genome130(), batch130(), libs, 70, A, 0, 1024)


@pytest.mark.parametrize("packed", [True, False])
def test_more_strata_than_one_launch_takes(packed):
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(libraries(1), 70, A, 0, lgd_max=1024, groups=genome130().names) as eng:
        eng.set_strata(np.arange(N130))
        eng.set_reference(genome130())
        eng.tabulate(batch130(), packed=packed)
        if packed:
            assert eng.packed_launches() == 3        # 64 + 64 + 2 (csrc/mdx_internal.h MDX_ML_MAX_LIBS)
        got = eng.finish()
    check(got, *want130())


def test_fewer_pools_than_strata(monkeypatch):
    from mapdamage_amd.engine import DamageEngine
    monkeypatch.setenv("MDX_TEST_CUS", "2")
    with DamageEngine(libraries(1), 70, A, 0, lgd_max=1024, groups=genome130().names) as eng:
        eng.set_strata(np.arange(N130))
        eng.set_reference(genome130())
        eng.tabulate(batch130(), packed=True)
        geom = eng.last_launch_geometry()
        assert 0 < geom["pools"] < N130, geom
        assert eng.packed_launches() >= -(-N130 // geom["pools"])
        got = eng.finish()
    check(got, *want130())


def test_more_strata_than_the_lds_counts():
    """2 libraries x 2 100 groups = 4 200 strata (csrc/mdx_internal.h LS_LDS_LIBS = 4 096): the tid key counts the kept
    records with global atomics.  5 000 records are two blocks of the key kernel (csrc/mdx_strata.hip STRATA_KEY_PER =
    4 096), the second one partial."""
    from mapdamage_amd.engine import DamageEngine
    ng, libs = 2100, libraries(2)
    group_of_tid = np.array([0, ng - 1, 1000, 17, ng - 2])
    b = batch5().slice(0, 5000)
    b.lib[:] = b.lib % 2
    filtered = (b.flag & 0xF04) != 0
    assert 10 < int(filtered.sum()) < b.n // 2 and filtered[4096:].any() and not filtered[4096:].all()
    want = np.bincount((b.lib.astype(np.int64) * ng + group_of_tid[b.tid])[~filtered], minlength=2 * ng).astype(np.uint64)
    assert np.count_nonzero(want) == 10
    with DamageEngine(libs, 70, A, 0, lgd_max=1024, groups=["g%d" % i for i in range(ng)]) as eng:
        eng.set_strata(group_of_tid)
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        eng.sync()
        np.testing.assert_array_equal(eng.strata_kept(), want)
        got = eng.finish()
    np.testing.assert_array_equal(got.kept, want)
    assert_tables_equal(got.merged, oracle_tableset(genome5(), b, libs, 70, A, 0, 1024))


# ---------------------------------------------------------------------- 4. memory
def _free(device=0):
    import torch
    torch.cuda.synchronize(device)
    return torch.cuda.mem_get_info(device)[0]


def test_a_thousand_strata_fit_and_one_library_keeps_its_copies():
    from mapdamage_amd.engine import DamageEngine
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    copy_bytes = 4 * 65536 * 8               # one library's dense histogram, one copy
    before = _free()
    with DamageEngine(libraries(1), 70, A, 0, groups=["g%d" % i for i in range(1000)]) as eng:
        used = before - _free()
        assert 1000 * copy_bytes <= used < 4 << 30, used
        assert eng.lgd_copies() == 1
        ref = genome5()
        eng.set_strata(np.arange(5) * 199)
        eng.set_reference(ref)
        b = batch5().slice(0, 5000)
        b.lib[:] = 0
        eng.tabulate(b, packed=True)
        eng.sync()
        kept = eng.strata_kept()
        assert int(kept.sum()) == int(((b.flag & 0xF04) == 0).sum()) and set(np.nonzero(kept)[0]) <= {0, 199, 398, 597, 796}
    before = _free()
    with DamageEngine(libraries(1), 70, A, 0) as eng:
        used = before - _free()
        assert eng.lgd_copies() == 32
        assert 32 * copy_bytes <= used < 1 << 30, used


# ---------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("packed", [True, False])
def test_a_kept_record_without_read_group_is_a_bad_read(packed):
    from mapdamage_amd.engine import BadReadError, DamageEngine
    b = batch5().slice(0, 3000)
    kept = np.nonzero((b.flag & 0xF04) == 0)[0]
    dropped = np.nonzero((b.flag & 0xF04) != 0)[0]
    b.lib[dropped[0]] = 0xFFFF               # (the flag filter drops it: no error)
    with DamageEngine(libraries(3), 70, A, 0, groups=["g0", "g1", "g2"]) as eng:
        eng.set_strata(GROUP_OF_TID)
        eng.set_reference(genome5())
        eng.tabulate(b, packed=packed)
        eng.reset()
        b.lib[kept[1234]] = 0xFFFF
        b.lib[kept[2000]] = 0xFFFF
        with pytest.raises(BadReadError) as err:
            eng.tabulate(b, packed=packed)
        assert err.value.read_index == int(kept[1234])


def _setters():
    """name -> a call of that setter on an engine of four tables that returns its code: four groups of every kind."""
    from mapdamage_amd import pmd
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)                    # noqa: E731
    tid = np.array([0, 1, 2, 3, 0], np.int32)
    off, start, end, group = np.array([0, 1, 1, 1, 1, 1], np.int64), np.array([10], np.int32), np.array([20], np.int32), np.array([0], np.int32)
    fx, terms = np.array([pmd.threshold_fx(t) for t in (0.0, 1.0, 2.0)], np.int64), np.ascontiguousarray(pmd.term_table(), np.int32)
    return {"mdx_set_strata": lambda e: e._lib.mdx_set_strata(e._ctx, 4, ptr(tid), 5),
            "mdx_set_strata_regions": lambda e: e._lib.mdx_set_strata_regions(e._ctx, 4, 5, ptr(off), ptr(start), ptr(end), ptr(group), 3),
            "mdx_set_strata_damage": lambda e: e._lib.mdx_set_strata_damage(e._ctx, 1, 0),
            "mdx_set_strata_pmd": lambda e: e._lib.mdx_set_strata_pmd(e._ctx, 3, ptr(fx), ptr(terms), 0)}


@pytest.mark.parametrize("first", ["mdx_set_strata", "mdx_set_strata_regions", "mdx_set_strata_damage", "mdx_set_strata_pmd"])
def test_a_context_has_one_kind_of_strata(first):
    """On a fresh context kind A is set; every other setter is a state error that names A's setter, and A again is allowed.
    (No record is counted, no kernel launched.)"""
    from mapdamage_amd.engine import DamageEngine
    from mapdamage_amd import layout as L
    setters = _setters()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c", "d"]) as eng:
        assert setters[first](eng) == 0 and eng._lib.mdx_strata_groups(eng._ctx) == 4
        for other, call in setters.items():
            if other != first:
                assert call(eng) == L.MDX_ERR_STATE, other
                message = eng._lib.mdx_last_error(eng._ctx).decode()
                assert "(%s)" % first in message and "one kind" in message, (other, message)
                assert eng._lib.mdx_strata_groups(eng._ctx) == 4
        assert setters[first](eng) == 0 and eng._lib.mdx_strata_groups(eng._ctx) == 4


def test_argument_and_state_errors():
    from mapdamage_amd.engine import DamageEngine, MdxConfig, MdxError
    from mapdamage_amd import layout as L
    with DamageEngine(libraries(3), 70, A, 0) as eng:       # three tables, two groups
        m = np.zeros(5, np.int32)
        rc = eng._lib.mdx_set_strata(eng._ctx, 2, ctypes.c_void_p(m.ctypes.data), 5)
        assert rc == L.MDX_ERR_ARG and b"no multiple" in eng._lib.mdx_last_error(eng._ctx)
    with DamageEngine(libraries(3), 70, A, 0, groups=["g0", "g1", "g2"]) as eng:
        with pytest.raises(MdxError) as err:
            eng.set_strata([0, 1, 3, 2, 1])                 # a group outside [0, n_groups)
        assert err.value.code == L.MDX_ERR_ARG
        eng.set_strata(GROUP_OF_TID)
        eng.set_reference(genome5())
        eng.tabulate(batch5().slice(0, 500), packed=True)
        with pytest.raises(MdxError) as err:
            eng.set_strata(GROUP_OF_TID)
        assert err.value.code == L.MDX_ERR_STATE
        # the fused tabulate-and-rescale calls count one library
        db = eng.upload(batch5().slice(0, 500), packed=False)
        rc = eng._lib.mdx_tabulate_rescale_device(eng._ctx, ctypes.byref(db.dev), None, None, None, None, None)
        assert rc == L.MDX_ERR_ARG and b"mdx_set_strata" in eng._lib.mdx_last_error(eng._ctx)
        db.free()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b"]) as eng:
        eng.set_strata([0, 1, 0])                           # three sequences, the reference has five
        eng.set_reference(genome5())
        with pytest.raises(MdxError) as err:
            eng.tabulate(batch5().slice(0, 500), packed=True)
        assert err.value.code == L.MDX_ERR_ARG
    # 70 000 strata: refused by the binding and by the library, each with a message
    with pytest.raises(ValueError, match="70000 tables"):
        DamageEngine(libraries(1), groups=["g%d" % i for i in range(70_000)])
    lib = eng._lib
    cfg, ctx = MdxConfig(70, A, 0, 70_000, 1024, 0, 16), ctypes.c_void_p()
    assert lib.mdx_create(ctypes.byref(cfg), ctypes.byref(ctx)) == L.MDX_ERR_ARG
    assert ctx.value and b"65535" in lib.mdx_last_error(ctx)
    lib.mdx_destroy(ctx)


# ---------------------------------------------------------------------- 6, 7. the command line
RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s1", "LB": "lib2"}]
CLI_LIBS = [("s1", "lib1"), ("s1", "lib2")]


@functools.lru_cache(maxsize=None)
def genome4():
    return synth.make_genome(seed=41, sizes=(("chr1", 8000), ("chr2", 4000), ("chrM", 2500), ("sc:1/*", 2000)), n_run=40, lower_run=200)


@functools.lru_cache(maxsize=None)
def batch4():
    return synth.make_reads(genome4(), 8000, 55, nlib=2, paired=True, **MIXED)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from mapdamage_amd import fasta, sam
    d = tmp_path_factory.mktemp("strata_cli")
    b, ref = batch4(), genome4()
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg)
    sam.write_sam(str(d / "in.sam"), b, ref.names, ref.lengths, RGS, rg)
    fasta.write_fasta(d / "ref.fa", ref)
    return d


def run_cli(d, out, *args):
    from mapdamage_amd.main import main
    assert main(["-r", str(d / "ref.fa"), "-d", str(out), "--no-stats"] + [str(a) for a in args]) == 0
    return out


def tree(folder):
    folder = str(folder)
    return {os.path.relpath(os.path.join(dp, f), folder): open(os.path.join(dp, f)).read()
            for dp, _, fs in os.walk(folder) for f in fs}


def check_tree(out, names, group_of_tid):
    groups, kept = yardstick(genome4(), batch4(), CLI_LIBS, group_of_tid, len(names), 70)
    files = tree(out / "by_reference")
    assert sorted(files) == sorted(["groups.tsv"] + ["%d/%s" % (g, f) for g in range(len(names)) for f in FILES])
    n_seq = np.bincount(group_of_tid, minlength=len(names))
    want = "Index\tGroup\tSequences\tReads\n" + "".join("%d\t%s\t%d\t%d\n" % (g, names[g], n_seq[g], groups[g].n_kept)
                                                         for g in range(len(names)))
    assert files["groups.tsv"] == want
    for g, t in enumerate(groups):
        assert files["%d/misincorporation.txt" % g] == t.misincorporation_text()
        assert files["%d/dnacomp.txt" % g] == t.dnacomp_text()
        assert files["%d/lgdistribution.txt" % g] == t.lgdistribution_text()


def test_command_line_three_routes(cli_files, tmp_path):
    d = cli_files
    plain = run_cli(d, tmp_path / "plain", "-i", d / "in.bam")
    assert not (plain / "by_reference").exists()
    outs = [run_cli(d, tmp_path / "bam", "-i", d / "in.bam", "--by-reference"),
            run_cli(d, tmp_path / "host", "-i", d / "in.bam", "--by-reference", "--host-decode"),
            run_cli(d, tmp_path / "sam", "-i", d / "in.sam", "--by-reference")]
    log = (outs[0] / "Runtime_log.txt").read_text()
    assert "GPU decode path gave up" not in log
    first = tree(outs[0] / "by_reference")
    for o in outs[1:]:
        assert tree(o / "by_reference") == first
    check_tree(outs[0], genome4().names, np.arange(4))
    for o in outs:
        for f in FILES:
            assert (o / f).read_text() == (plain / f).read_text(), (o, f)
    # groups of sequences: two named ones, the rest in '*'
    (tmp_path / "g.tsv").write_text("chrM\tmito\nchr2\tnuclear\nchr1\tnuclear\n")
    grouped = run_cli(d, tmp_path / "grouped", "-i", d / "in.bam", "--reference-groups", tmp_path / "g.tsv")
    check_tree(grouped, ["mito", "nuclear", "*"], np.asarray([1, 1, 0, 2]))
    for f in FILES:
        assert (grouped / f).read_text() == (plain / f).read_text(), f
    # a name the header lacks: an error that names it, no tables
    (tmp_path / "bad.tsv").write_text("chrM\tmito\nchrQ\tnuclear\n")
    from mapdamage_amd.main import main
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / "bad"), "--reference-groups",
                 str(tmp_path / "bad.tsv")]) == 1
    assert "chrQ" in (tmp_path / "bad" / "Runtime_log.txt").read_text()


def test_two_ranks_write_the_same_tree(cli_files, tmp_path):
    """``--gpus 2`` against ``--gpus 1``, each a process of its own (one that has not touched the GPU before the run does)."""
    d = cli_files
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    # (several slabs out of a small file: both ranks decode and count)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1", MDX_GBAM_SLAB_BYTES="65536")
    for name, extra in (("one", []), ("two", ["--gpus", "2", "--share-gpu", "--dist-backend", "gloo"])):
        cmd = [sys.executable, "-m", "mapdamage_amd", "-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / name),
               "--no-stats", "--by-reference"] + extra
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    check_tree(tmp_path / "one", genome4().names, np.arange(4))
    assert tree(tmp_path / "two" / "by_reference") == tree(tmp_path / "one" / "by_reference")
    for f in FILES:
        assert (tmp_path / "two" / f).read_text() == (tmp_path / "one" / f).read_text(), f
