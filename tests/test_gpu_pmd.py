"""Strata by post-mortem damage score on the device: tables per (library, interval of the score) from one pass, and the score
histogram (include/mdx.h ``mdx_set_strata_pmd``, ``mdx_strata_pmd_histogram``; ``--by-pmd-score``).

The yardstick shares nothing with the product: a record's score is the restatement's (tests/pmd_util.py — the two gapped
strings, the formulas' table), the group tables are tests/test_gpu_regions.py's ``yardstick`` — one oracle run per stratum —
and the comparison tests/test_gpu_strata.py's ``check``.  The key column itself stays inside the library; what it decides —
the kept reads per stratum, the tables per group — and the histogram are compared exactly.  tests/test_pmd.py checks on the
CPU that every input of ``inputs()`` fills all its groups and ten bins."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import layout as L
from mapdamage_amd import pmd
from mapdamage_amd.batch import concat_batches
from tests import pmd_util as P
from tests.test_gpu_regions import brute_kept, run, yardstick
from tests.test_gpu_strata import A, CLI_LIBS, FILES, RGS, check, genome4, genome5, libraries, tree
from tests.util import oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRATA_KEY_PER = 4096           # csrc/mdx_strata.hip: the records of one block of the key kernel
THS3 = (0.0, 1.5, 3.0)


# ---------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def mixed():
    """The hand-made records (the degenerate ones dropped by flag 0x200: the tabulation reports a kept one) in front of
    3 000 synthetic ones of 30 to 160 bases — shorter than, as long as and several times the 16 lanes that share a record."""
    b = concat_batches([P.hand_batch(genome5(), "dropped"), P.synthetic_batch(genome5(), 3000, 31, 3)])
    lens = np.diff(b.seq_off.astype(np.int64))
    assert (lens < 16).any() and (lens == 30).any() and (lens > 150).any() and len(set((lens % 16).tolist())) == 16
    return b


@functools.lru_cache(maxsize=None)
def one_library():
    b = mixed().slice(0, mixed().n)
    b.lib[:] = 0
    return b


@functools.lru_cache(maxsize=None)
def key_per():
    """One record more than a block of the key kernel takes, short (the restatement walks them in Python)."""
    return P.synthetic_batch(genome5(), STRATA_KEY_PER + 1, 33, 3, len_range=(30, 70))


@functools.lru_cache(maxsize=None)
def cli_batch():
    """Two libraries over ``genome4()``, with qualities but for forty records."""
    b = P.synthetic_batch(genome4(), 4000, 57, 2, len_range=(30, 140))
    for i in range(0, 4000, 100):
        b.qual[int(b.seq_off[i]):int(b.seq_off[i + 1])] = 0xFF
    return b


def inputs():
    """name -> (reference, batch, libraries, thresholds, single-stranded) of every test below."""
    many = key_per().slice(0, 3000)
    many.lib[:] = (np.arange(3000) * 7 % 2100).astype(np.uint16)
    sixty = key_per().slice(0, 3000)
    sixty.lib[:] = (np.arange(3000) % 60).astype(np.uint16)
    return {"mixed": (genome5(), mixed(), 3, THS3, False),
            "mixed, single-stranded": (genome5(), mixed(), 3, THS3, True),
            "one library": (genome5(), one_library(), 1, (3.0,), False),
            "key per": (genome5(), key_per(), 3, (3.0,), False),
            "first 255 of key per": (genome5(), key_per().slice(0, 255), 3, (3.0,), False),
            "2100 libraries": (genome5(), many, 2100, (3.0,), False),
            "60 libraries": (genome5(), sixty, 60, (3.0,), False),
            "command line": (genome4(), cli_batch(), 2, (0.0, 3.0), False)}


@functools.lru_cache(maxsize=None)
def S_of(name, with_qual=True):
    ref, b, _, _, single_stranded = inputs()[name]
    if not with_qual:
        b = b.slice(0, b.n)
        b.qual = None
    return P.scores(ref, b, single_stranded)


def pmd_engine(libs, thresholds, single_stranded=False, length=70, minqual=0, **kw):
    from mapdamage_amd.engine import DamageEngine
    eng = DamageEngine(libs, length, A, minqual, groups=pmd.group_names(thresholds), **kw)
    eng.set_strata_pmd(thresholds, single_stranded=single_stranded)
    return eng


def check_counts(eng, b, S, nlib, thresholds, times=1):
    """The kept reads per stratum and the histogram against the restatement, and the invariant that ties them."""
    ng = len(thresholds) + 1
    kept, hist = eng.strata_kept(), eng.pmd_histogram()
    np.testing.assert_array_equal(kept, times * brute_kept(b, P.groups_of(S, thresholds), nlib, ng))
    np.testing.assert_array_equal(hist, times * P.histogram(b, S, nlib))
    np.testing.assert_array_equal(hist.sum(axis=1), kept.reshape(nlib, ng).sum(axis=1))
    keep = (b.flag & 0xF04) == 0
    assert int(kept.sum()) == times * int(keep.sum())
    first = np.minimum(b.seq_off[:-1].astype(np.int64), max(0, b.seq.shape[0] - 1))
    no_qual = np.ones(b.n, bool) if b.qual is None else (np.diff(b.seq_off.astype(np.int64)) == 0) | (b.qual[first] == 0xFF)
    assert eng.pmd_unqualified() == times * int((keep & no_qual).sum())


# ---------------------------------------------------------------------- 1. batch sizes, SEQ forms, with and without qualities
@pytest.mark.parametrize("with_qual", [True, False])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, STRATA_KEY_PER - 1, STRATA_KEY_PER, STRATA_KEY_PER + 1])
def test_kept_counts_and_histogram_at_the_sizes_where_the_kernel_turns(n, packed, with_qual):
    b = key_per().slice(0, n)
    S = S_of("key per", with_qual)[:n]
    if not with_qual:
        b.qual = None
    with pmd_engine(libraries(3), (3.0,)) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=packed)
        check_counts(eng, b, S, 3, (3.0,))
    if n > 1:
        assert (S_of("key per", True)[:n] != S_of("key per", False)[:n]).any()


# ---------------------------------------------------------------------- 2. the tables per group, both routes
@functools.lru_cache(maxsize=None)
def want_tables(name):
    ref, b, nlib, ths, _ = inputs()[name]
    group = P.groups_of(S_of(name), ths)
    groups, kept = yardstick(ref, b, libraries(nlib), group, len(ths) + 1, 70)
    np.testing.assert_array_equal(kept, brute_kept(b, group, nlib, len(ths) + 1))
    return groups, kept, oracle_tableset(ref, b, libraries(nlib), 70, A, 0)


@pytest.mark.parametrize("form", ["packed", "ascii", "resident"])
def test_tables_per_group_three_libraries_four_groups(form):
    b = mixed()
    with pmd_engine(libraries(3), THS3) as eng:
        eng.set_reference(genome5())
        lib_before = b.lib.copy()
        run(eng, b, form)
        assert eng.packed_launches() == (0 if form == "ascii" else 1)
        check_counts(eng, b, S_of("mixed"), 3, THS3)
        got = eng.finish()
        np.testing.assert_array_equal(b.lib, lib_before)
    assert got.groups == ["<0", "[0,1.5)", "[1.5,3)", ">=3"]
    check(got, *want_tables("mixed"))
    np.testing.assert_array_equal(got.pmd_hist, P.histogram(b, S_of("mixed"), 3))


def test_tables_per_group_one_library_two_groups():
    b = one_library()
    with pmd_engine(libraries(1), (3.0,)) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        check_counts(eng, b, S_of("one library"), 1, (3.0,))
        got = eng.finish()
    check(got, *want_tables("one library"))


def test_a_resident_batch_tabulated_twice_keeps_the_histogram_in_step():
    """``mdx_batch_upload`` buckets the batch by the key; its tabulations take the kept counts from the buckets and launch
    the key kernel for the histogram alone."""
    b = mixed()
    with pmd_engine(libraries(3), THS3) as eng:
        eng.set_reference(genome5())
        db = eng.upload(b, packed=True)
        assert not eng.strata_kept().any() and not eng.pmd_histogram().any()       # (uploading counts nothing)
        for times in (1, 2):
            eng.tabulate(db)
            eng.sync()
            check_counts(eng, b, S_of("mixed"), 3, THS3, times)
        assert eng.libsorts() == 0
        got = eng.finish()
        db.free()
        groups, kept, whole = want_tables("mixed")
        np.testing.assert_array_equal(got.merged.mis, 2 * whole.mis)
        for g in range(4):
            np.testing.assert_array_equal(got.group(g).mis, 2 * groups[g].mis)
        # reset clears the histogram with the kept counts
        eng.reset()
        assert not eng.strata_kept().any() and not eng.pmd_histogram().any() and eng.pmd_unqualified() == 0


def test_single_stranded():
    b = mixed()
    assert (S_of("mixed") != S_of("mixed, single-stranded")).sum() > 1000
    with pmd_engine(libraries(3), THS3, single_stranded=True) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        check_counts(eng, b, S_of("mixed, single-stranded"), 3, THS3)


def test_a_small_device(monkeypatch):
    """MDX_TEST_CUS (tests/test_gpu_few_cus.py): the launches sized as on a device of two compute units."""
    monkeypatch.setenv("MDX_TEST_CUS", "2")
    b = mixed()
    with pmd_engine(libraries(3), THS3) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        check_counts(eng, b, S_of("mixed"), 3, THS3)
        check(eng.finish(), *want_tables("mixed"))


@pytest.mark.parametrize("knob", ["MDX_PMD_LANE", "MDX_PMD_NO_LDS"])
def test_the_kernels_kept_for_measurements_give_the_same(monkeypatch, knob):
    """MDX_PMD_LANE=1: a lane per record instead of sixteen; MDX_PMD_NO_LDS=1: sixteen lanes, every term from global memory
    (what tools/strata_cost.py measures the kernel against)."""
    monkeypatch.setenv(knob, "1")
    b = mixed()
    with pmd_engine(libraries(3), THS3) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        check_counts(eng, b, S_of("mixed"), 3, THS3)


# ---------------------------------------------------------------------- 3. more strata and bins than the LDS counts
@pytest.mark.parametrize("name,nl", [("2100 libraries", 2100), ("60 libraries", 60)])
def test_more_strata_and_bins_than_the_lds_counts(name, nl):
    """2 100 libraries x 2 groups = 4 200 strata (csrc/mdx_internal.h LS_LDS_LIBS = 4 096): kept reads and histogram
    through global atomics; 60 libraries: 4 921 histogram words (PMD_HIST_LDS = 4 096) beside strata counted in the LDS."""
    _, b, _, ths, _ = inputs()[name]
    libs = [("S%d" % i, "L") for i in range(nl)]
    with pmd_engine(libs, ths, length=20, lgd_max=512) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        check_counts(eng, b, S_of(name), nl, ths)
        got = eng.finish()
    b1 = b.slice(0, b.n)
    b1.lib[:] = 0
    whole = oracle_tableset(genome5(), b1, libraries(1), 20, A, 0, 512)
    np.testing.assert_array_equal(got.merged.mis.sum(axis=0), whole.mis[0])
    assert int(got.kept.sum()) == got.n_kept


# ---------------------------------------------------------------------- 4. dropped and degenerate records
def test_dropped_records_are_counted_nowhere():
    b = mixed()
    dropped = (b.flag & 0xF04) != 0
    assert (b.flag & 0x200).any() and (b.flag & 0x4).any() and dropped.sum() > 50
    only = b.take(np.flatnonzero(dropped))
    with pmd_engine(libraries(3), THS3) as eng:
        eng.set_reference(genome5())
        eng.tabulate(only, packed=True)
        assert not eng.strata_kept().any() and not eng.pmd_histogram().any() and eng.pmd_unqualified() == 0


def test_a_kept_degenerate_record_scores_zero_and_is_reported():
    from mapdamage_amd.engine import BadReadError
    b = P.hand_batch(genome5(), "kept")
    names = [row[0] for row in P.HAND + P.DEGENERATE]
    for name in ("tid outside the reference", "window past the contig's end"):
        i = names.index(name)
        with pmd_engine(libraries(2), (-1.0, 0.0, 3.0)) as eng:
            eng.set_reference(genome5())
            with pytest.raises(BadReadError):
                eng.tabulate(b.slice(i, i + 1), packed=True)
            # S = 0: two thresholds reached, the bin that begins at 0
            want = np.zeros(8, np.uint64)
            want[int(b.lib[i]) * 4 + 2] = 1
            np.testing.assert_array_equal(eng.strata_kept(), want)
            assert eng.pmd_histogram()[int(b.lib[i]), 41] == 1 and eng.pmd_histogram().sum() == 1


# ---------------------------------------------------------------------- 5. the rules of the calls
def _set(eng, thresholds, terms="default", single_stranded=0):
    fx = np.array([pmd.threshold_fx(t) for t in thresholds], np.int64)
    if isinstance(terms, str):
        terms = np.ascontiguousarray(pmd.term_table())
    rc = eng._lib.mdx_set_strata_pmd(eng._ctx, len(thresholds), None if not len(fx) else fx.ctypes.data_as(ctypes.c_void_p),
                                     None if terms is None else terms.ctypes.data_as(ctypes.c_void_p), single_stranded)
    return rc, eng._lib.mdx_last_error(eng._ctx).decode()


def test_argument_and_state_errors():
    from mapdamage_amd.engine import DamageEngine, MdxError
    b = key_per().slice(0, 500)
    hist = np.zeros(82 * 4, np.uint64)
    with DamageEngine(libraries(3), 70, A, 0) as eng:                # three tables: no multiple of two groups
        rc, msg = _set(eng, [3.0])
        assert rc == L.MDX_ERR_ARG and "no multiple" in msg
        # no PMD strata: the histogram is a state error
        assert eng._lib.mdx_strata_pmd_histogram(eng._ctx, hist.ctypes.data_as(ctypes.c_void_p)) == L.MDX_ERR_STATE
        assert eng._lib.mdx_strata_pmd_unqualified(eng._ctx, hist.ctypes.data_as(ctypes.c_void_p)) == L.MDX_ERR_STATE
        with pytest.raises(MdxError):
            eng.pmd_histogram()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c", "d"]) as eng:
        for ths, word in (([], "thresholds"), (list(range(16)), "thresholds"), ([0.0, 3.0, 3.0], "increasing"), ([3.0, 0.0, 5.0], "increasing")):
            rc, msg = _set(eng, ths)
            assert rc == L.MDX_ERR_ARG and word in msg, (ths, rc, msg)
        rc, msg = _set(eng, [0.0, 1.0, 2.0], terms=None)
        assert rc == L.MDX_ERR_ARG and "null" in msg
        rc, msg = _set(eng, [0.0, 1.0])                              # three groups into four tables
        assert rc == L.MDX_ERR_ARG and "no multiple" in msg
        assert eng._lib.mdx_strata_groups(eng._ctx) == 0
        assert eng._lib.mdx_strata_pmd_histogram(eng._ctx, None) == L.MDX_ERR_ARG
        rc, msg = _set(eng, [0.0, 1.0, 2.0], single_stranded=1)
        assert rc == 0, msg
        assert eng._lib.mdx_strata_groups(eng._ctx) == 4
        rc, msg = _set(eng, [3.0])                                   # again, with other thresholds: four tables, two groups
        assert rc == 0 and eng._lib.mdx_strata_groups(eng._ctx) == 2 and eng.pmd_histogram().shape == (2, 82)
        rc, msg = _set(eng, [0.0, 1.0, 2.0])
        assert rc == 0
        # PMD strata, then each other kind: one kind per context
        with pytest.raises(MdxError) as err:
            eng.set_strata([0, 1, 2, 3, 0])
        assert err.value.code == L.MDX_ERR_STATE and "mdx_set_strata_pmd" in str(err.value)
        with pytest.raises(MdxError) as err:
            eng.set_strata_regions([0, 1, 1, 1, 1, 1], [10], [20], [0])
        assert err.value.code == L.MDX_ERR_STATE and "mdx_set_strata_pmd" in str(err.value)
        rc = eng._lib.mdx_set_strata_damage(eng._ctx, 1, 0)
        assert rc == L.MDX_ERR_STATE and b"mdx_set_strata_pmd" in eng._lib.mdx_last_error(eng._ctx)
        # the key reads the reference: upload and tabulation before it are refused, with a message that says so
        for packed in (True, False):
            with pytest.raises(MdxError) as err:
                eng.upload(b, packed=packed)
            assert err.value.code == L.MDX_ERR_STATE and "reference" in str(err.value)
        with pytest.raises(MdxError) as err:
            eng.tabulate(b, packed=True)
        assert err.value.code == L.MDX_ERR_STATE and "reference" in str(err.value)
    # ... and this kind after each of the others
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c", "d"]) as eng:
        eng.set_strata([0, 1, 2, 3, 0])
        rc, msg = _set(eng, [0.0, 1.0, 2.0])
        assert rc == L.MDX_ERR_STATE and "(mdx_set_strata)" in msg
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c", "d"]) as eng:
        eng.set_strata_regions([0, 1, 1, 1, 1, 1], [10], [20], [0])
        rc, msg = _set(eng, [0.0, 1.0, 2.0])
        assert rc == L.MDX_ERR_STATE and "mdx_set_strata_regions" in msg
    with DamageEngine(libraries(1), 70, A, 0, groups=["none", "5p", "3p", "both"]) as eng:
        eng.set_strata_damage(1)
        rc, msg = _set(eng, [0.0, 1.0, 2.0])
        assert rc == L.MDX_ERR_STATE and "mdx_set_strata_damage" in msg
    # a context with a --min-basequal
    with DamageEngine(libraries(1), 70, A, 20, groups=["a", "b"]) as eng:
        rc, msg = _set(eng, [3.0])
        assert rc == L.MDX_ERR_ARG and "min-basequal" in msg
    with pmd_engine(libraries(3), (3.0,)) as eng:
        eng.set_reference(genome5())
        eng.tabulate(b, packed=True)
        rc, msg = _set(eng, [3.0])                                   # the setter after a tabulation
        assert rc == L.MDX_ERR_STATE and "counted" in msg
        db = eng.upload(b, packed=False)
        rc = eng._lib.mdx_tabulate_rescale_device(eng._ctx, ctypes.byref(db.dev), None, None, None, None, None)
        assert rc == L.MDX_ERR_ARG and b"mdx_set_strata" in eng._lib.mdx_last_error(eng._ctx)
        db.free()
    with DamageEngine(libraries(1), 70, A, 0, groups=["a", "b", "c"]) as eng:
        with pytest.raises(ValueError, match="groups"):
            eng.set_strata_pmd([3.0])
        with pytest.raises(ValueError, match="increasing"):
            eng.set_strata_pmd([3.0, 1.0])
    with DamageEngine(libraries(1), 70, A, 0) as eng:
        with pytest.raises(ValueError, match="groups"):
            eng.set_strata_pmd([3.0])


# ---------------------------------------------------------------------- 6. the command line
CLI_THS = (0.0, 3.0)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from mapdamage_amd import fasta, sam
    from tests.test_fasta_bgzf import _bgzip
    d = tmp_path_factory.mktemp("pmd_cli")
    b, ref = cli_batch(), genome4()
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg)
    sam.write_sam(str(d / "in.sam"), b, ref.names, ref.lengths, RGS, rg)
    _bgzip(d / "in.sam", d / "in.sam.gz")
    fasta.write_fasta(d / "ref.fa", ref)
    return d


@functools.lru_cache(maxsize=None)
def cli_want():
    S = S_of("command line")
    group = P.groups_of(S, CLI_THS)
    return yardstick(genome4(), cli_batch(), CLI_LIBS, group, 3, 70)[0], P.histogram(cli_batch(), S, 2)


def check_tree(out):
    groups, hist = cli_want()
    files = tree(out / "by_pmd")
    assert sorted(files) == sorted(["groups.tsv", "scores.tsv"] + ["%d/%s" % (g, f) for g in range(3) for f in FILES])
    assert files["groups.tsv"] == "Index\tGroup\tReads\n" + "".join("%d\t%s\t%d\n" % (g, name, groups[g].n_kept)
                                                                   for g, name in enumerate(["<0", "[0,3)", ">=3"]))
    for g, t in enumerate(groups):
        assert files["%d/misincorporation.txt" % g] == t.misincorporation_text()
        assert files["%d/dnacomp.txt" % g] == t.dnacomp_text()
        assert files["%d/lgdistribution.txt" % g] == t.lgdistribution_text()
    assert files["scores.tsv"] == P.scores_tsv(CLI_LIBS, hist)


def run_cli(d, out, *args):
    from mapdamage_amd.main import main
    assert main(["-r", str(d / "ref.fa"), "-d", str(out), "--no-stats"] + [str(a) for a in args]) == 0
    return out


EXTRA = ["--by-pmd-score", "--pmd-thresholds", "0,3"]


def test_command_line_four_routes(cli_files, tmp_path):
    d = cli_files
    plain = run_cli(d, tmp_path / "plain", "-i", d / "in.bam")
    assert not (plain / "by_pmd").exists()
    outs = [run_cli(d, tmp_path / "bam", "-i", d / "in.bam", *EXTRA),
            run_cli(d, tmp_path / "sam", "-i", d / "in.sam", *EXTRA),
            run_cli(d, tmp_path / "samgz", "-i", d / "in.sam.gz", *EXTRA),
            run_cli(d, tmp_path / "host", "-i", d / "in.bam", "--host-decode", *EXTRA)]
    b = cli_batch()
    no_qual = int((((b.flag & 0xF04) == 0) & (b.qual[b.seq_off[:-1]] == 0xFF)).sum())
    assert 30 <= no_qual <= 40
    for o in outs:
        log = (o / "Runtime_log.txt").read_text()
        assert "GPU decode path gave up" not in log
        assert "PMD scores: %d records without PHRED scores were scored with a base error of 0" % no_qual in log, o
        check_tree(o)
        for f in FILES:
            assert (o / f).read_text() == (plain / f).read_text(), (o, f)
    check_usual_files(plain)
    assert "inflated and parsed on the device" in (outs[2] / "Runtime_log.txt").read_text()
    # the default threshold is 3
    one = run_cli(d, tmp_path / "one", "-i", d / "in.bam", "--by-pmd-score")
    S = S_of("command line")
    keep = (cli_batch().flag & 0xF04) == 0
    assert (one / "by_pmd" / "groups.tsv").read_text() == "Index\tGroup\tReads\n0\t<3\t%d\n1\t>=3\t%d\n" % (
        int((keep & (S < 3 << 24)).sum()), int((keep & (S >= 3 << 24)).sum()))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def check_usual_files(out):
    """The three usual files are those of the run without the option: the oracle's over the untouched batch (which
    test_command_line_four_routes holds the plain run's files to as well)."""
    want = oracle_tableset(genome4(), cli_batch(), CLI_LIBS, 70, A, 0)
    assert (out / "misincorporation.txt").read_text() == want.misincorporation_text()
    assert (out / "dnacomp.txt").read_text() == want.dnacomp_text()
    assert (out / "lgdistribution.txt").read_text() == want.lgdistribution_text()


def check_chains(out):
    """A ``--stats --fix-nicks`` run has written a chain's three files into every group directory that has data (a C at the
    first 5p position and a G at the first 3p one), into no other, and beside the usual files."""
    from tests.test_gpu_stats import CSVS
    groups, _ = cli_want()
    with_data = 0
    for g, t in enumerate(groups):
        has_data = bool(t.mis[:, L.ENDS.index("5p"), :, 0, L.MIS_COLS.index("C")].sum()) and \
            bool(t.mis[:, L.ENDS.index("3p"), :, 0, L.MIS_COLS.index("G")].sum())
        assert all((out / "by_pmd" / str(g) / name).is_file() == has_data for name in CSVS), (out, g)
        with_data += has_data
    assert with_data >= 2 and all((out / name).is_file() for name in CSVS)


def check_tree_with_chains(out):
    """``check_tree`` of a run with ``--stats``: the chains' files are beside the tables."""
    from tests.test_gpu_stats import CSVS
    files = {k: v for k, v in tree(out / "by_pmd").items() if os.path.basename(k) not in CSVS}
    assert sorted(files) == sorted(["groups.tsv", "scores.tsv"] + ["%d/%s" % (g, f) for g in range(3) for f in FILES])
    groups, hist = cli_want()
    for g, t in enumerate(groups):
        assert files["%d/misincorporation.txt" % g] == t.misincorporation_text()
        assert files["%d/dnacomp.txt" % g] == t.dnacomp_text()
        assert files["%d/lgdistribution.txt" % g] == t.lgdistribution_text()
    assert files["scores.tsv"] == P.scores_tsv(CLI_LIBS, hist)
    check_usual_files(out)
    check_chains(out)


def test_command_line_from_stdin(cli_files, tmp_path):
    """One run with ``--stats --fix-nicks``: the tree, the usual files and the chains of the stream route."""
    from tests.test_gpu_stats import FAST
    d = cli_files
    cmd = [sys.executable, "-m", "mapdamage_amd", "-i", "-", "-r", str(d / "ref.fa"), "-d", str(tmp_path / "pipe"), "--stats"] + EXTRA + FAST
    out = subprocess.run(cmd, cwd=ROOT, env=_env(), input=(d / "in.bam").read_bytes(), capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr[-6000:]
    assert "from a stream" in (tmp_path / "pipe" / "Runtime_log.txt").read_text()
    check_tree_with_chains(tmp_path / "pipe")


def test_two_ranks_write_the_same_tree(cli_files, tmp_path):
    from tests.test_gpu_stats import FAST
    d = cli_files
    env = _env()
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1", MDX_GBAM_SLAB_BYTES="65536")
    cmd = [sys.executable, "-m", "mapdamage_amd", "-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(tmp_path / "two"),
           "--stats", "--gpus", "2", "--share-gpu", "--dist-backend", "gloo"] + EXTRA + FAST
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    check_tree_with_chains(tmp_path / "two")


@pytest.mark.parametrize("route", ["bam", "sam", "samgz", "host"])
def test_stats_writes_a_chain_into_every_group_with_data(cli_files, tmp_path, route):
    from mapdamage_amd.main import main
    from tests.test_gpu_stats import FAST
    d = cli_files
    source = {"bam": ["-i", str(d / "in.bam")], "sam": ["-i", str(d / "in.sam")], "samgz": ["-i", str(d / "in.sam.gz")],
              "host": ["-i", str(d / "in.bam"), "--host-decode"]}[route]
    out = tmp_path / "stats"
    assert main(source + ["-r", str(d / "ref.fa"), "-d", str(out), "--stats"] + EXTRA + FAST) == 0
    check_tree_with_chains(out)
