"""--pileup-damage-profile on the device (mapdamage_amd/csrc/mdx_pileup.hip): the 20 sums per site, the ten values, the best
genotype and the bases of ``pileup_likelihoods_finish`` behind ``pileup_likelihoods_damage_begin`` over the small BAM files of
tests/test_gpu_pileup.py against the brute force of tests/gld_rule.py, ``==`` — the hand-written table, dense sites where the add
kernel's list turns, batches around the block size, contended 64-bit atomics, reads shorter than K and reads that reach the tail,
one slab and many, the state rules —, and the command line's files against the rule's.  The rule on the host, the profile, the
table and the emitters: tests/test_pileup_damage_likelihoods.py."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gl_rule as GR
from tests import gld_rule as DR
from tests import pileup_rule as PR
from tests.test_gpu_depth import names_of, reference
from tests.test_gpu_pileup import (DENSE_LENGTHS, DENSE_SITES, ERR_STATE, add_file, begin, check, clustered, dense_records, engine, exact_records,  # noqa: F401
                                   expected_files, panel, site_columns, spread, turns, write_records)
from tests.test_gpu_pileup_likelihoods import expected_likelihoods
from tests.test_gpu_remove_duplicates import LIBS3, dup_data      # noqa: F401  (dup_data: a fixture)
from tests.test_gpu_write_kept import DEVICE, run, tables
from tests.test_pileup import HAND_LENGTHS, HAND_LIBRARIES, HAND_RECORDS, HAND_SETTINGS, HAND_SITES, rec
from tests.test_pileup_damage_likelihoods import D3_K5, D3_K20, D5_K5, D5_K20, ROWS3, ROWS5, TEXT, special_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, P, EQ, X = range(9)
DENSE_NOQUAL = 17
PROFILES = {5: (D5_K5, D3_K5), 20: (D5_K20, D3_K20)}
_tables = {}


def table_of(k):
    """The package's table of the test profile with K = ``k`` (tests/test_pileup_damage_likelihoods.py holds it to the brute force's)."""
    from mapdamage_amd import pileup
    if k not in _tables:
        _tables[k] = pileup.damage_likelihood_table(pileup.parse_damage_profile(TEXT.split("\n"), k))
    return _tables[k]


def check_gld(got, records, lengths, sites, k, n_libraries=3, k5=0, k3=0, min_qual=0, noqual=30, alleles=None, single_strand=False):
    """What ``pileup_likelihoods_finish`` gave against the rule: every sum, every value, the best and the bases bit for bit."""
    sums, gl, best, bases, counts = got
    d5, d3 = PROFILES[k]
    counters, _ = PR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual)
    want_sums, want_counts = DR.brute(records, n_libraries, lengths, sites, DR.rates(d5), DR.rates(d3), k5, k3, min_qual, noqual)
    want_gl, want_best, want_bases = DR.all_likelihoods(want_sums, counters, alleles, single_strand)
    want_sums = np.array(want_sums, np.int64).reshape(-1, 20)
    assert sums.shape == want_sums.shape and sums.dtype == np.int64 and gl.shape == want_gl.shape and gl.dtype == np.int64
    assert (sums == want_sums).all(), [(sites[g], sums[g].tolist(), want_sums[g].tolist()) for g in np.flatnonzero((sums != want_sums).any(axis=1))[:3]]
    assert (gl == want_gl).all(), [(sites[g], gl[g].tolist(), want_gl[g].tolist()) for g in np.flatnonzero((gl != want_gl).any(axis=1))[:3]]
    assert best.dtype == np.uint8 and best.tolist() == want_best and bases.dtype == np.uint32 and bases.tolist() == want_bases
    assert counts == want_counts, (counts, want_counts)
    return want_sums, want_gl, want_best, want_bases, want_counts


# ---------------------------------------------------------------------- 1. the rule on the device
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "ascii"])
def test_hand_written_records_on_the_device(engine, tmp_path, packed):
    write_records(tmp_path / "in.bam", HAND_RECORDS, names_of(HAND_LENGTHS + [50]), HAND_LENGTHS + [50])
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(HAND_SITES))]
    for n, (k5, k3, q) in enumerate(HAND_SETTINGS):
        k = (5, 20)[n % 2]
        options = dict(mode=("random", "majority", "none")[n % 3], seed=n, min_depth=1 + n % 2, single_strand=bool(n % 2))
        noqual = (30, 7, 93, 1)[n % 4]
        ref = begin(engine, HAND_LENGTHS, HAND_SITES, alleles, min_basequal=q, mask_ends=(k5, k3), call=options["mode"], seed=n,
                    min_depth=options["min_depth"], single_strand=options["single_strand"])
        plain = engine.pileup_info()["bytes"]
        engine.pileup_likelihoods_damage_begin(table_of(k), noqual_quality=noqual)
        assert engine.pileup_info()["bytes"] == plain + len(HAND_SITES) * 160 + 2 * (k + 1) * 94 * 9 * 8 + 16
        assert add_file(engine, tmp_path / "in.bam", packed=packed) == [len(HAND_RECORDS)]
        check_gld(engine.pileup_likelihoods_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, k, HAND_LIBRARIES, k5, k3, q, noqual, alleles, options["single_strand"])
        check(engine.pileup_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, ref, HAND_LIBRARIES, k5, k3, q, alleles=alleles, **options)
    assert engine.pileup_likelihoods_finish(with_sums=False)[0] is None


# ---------------------------------------------------------------------- 2. dense sites: the list's rounds
def test_dense_sites_with_the_whole_list(engine, turns, tmp_path):
    records = dense_records()
    write_records(tmp_path / "in.bam", records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    begin(engine, DENSE_LENGTHS, DENSE_SITES, min_basequal=20, mask_ends=(1, 0), call="majority", seed=3)
    engine.pileup_likelihoods_damage_begin(table_of(5), noqual_quality=DENSE_NOQUAL)
    assert add_file(engine, tmp_path / "in.bam") == [2000]
    _, _, best, bases, counts = check_gld(engine.pileup_likelihoods_finish(), records, DENSE_LENGTHS, DENSE_SITES, 5, k5=1, k3=0, min_qual=20, noqual=DENSE_NOQUAL)
    assert counts["added"] > 20_000 > turns["list"] and counts["without_qualities"] > 1000 and max(bases) > 100 and len(set(best)) >= 4


# ---------------------------------------------------------------------- 3. a list of 48 pairs
@pytest.fixture(scope="module")
def small_list(tmp_path_factory):
    """A child process whose add kernel's list holds 48 pairs, as in tests/test_gpu_pileup.py, with the damage sums beside the
    counters: a round ends inside a record's pairs in `dense`, `over` and `alone`."""
    d = tmp_path_factory.mktemp("pileup_gld_list")
    cases = {"dense": dense_records(), "exact": exact_records(48), "over": exact_records(49), "twice": exact_records(96),
             "alone": [rec(0x10, 0, 0, 20, [(M, 250)], "CTGAT" * 50)]}
    for name, records in cases.items():
        write_records(d / (name + ".bam"), records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_pileup_gld_worker.py"), str(d)] + sorted(cases), cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_PILEUP_LIST="48"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    return d, cases


@pytest.mark.parametrize("case", ["dense", "exact", "over", "twice", "alone"])
def test_pairs_where_the_list_turns(small_list, case):
    d, cases = small_list
    z = np.load(d / (case + ".npz"))
    assert int(z["info"][0]) == 48
    added = dict(zip(("added", "without_qualities"), (int(x) for x in z["added"])))
    check_gld((z["sums"], z["gl"], z["best"], z["bases"], added), cases[case], DENSE_LENGTHS, DENSE_SITES, 5, k5=1, k3=0, min_qual=20, noqual=DENSE_NOQUAL)
    counts = dict(zip(("counted", "outside", "over_a_site", "pairs"), (int(x) for x in z["counts"])))
    _, want_counts = check((z["counters"], z["refbase"], z["call"], z["depth"], counts), cases[case], DENSE_LENGTHS, DENSE_SITES, reference(DENSE_LENGTHS),
                           k5=1, k3=0, min_qual=20, mode="majority", seed=3)
    assert want_counts["pairs"] == {"exact": 48, "over": 49, "twice": 96, "alone": 250}.get(case, want_counts["pairs"])


# ---------------------------------------------------------------------- 4. batches around the block size
@pytest.mark.parametrize("size", ["block-1", "block", "block+1"])
def test_record_counts_where_the_add_kernel_turns(engine, turns, tmp_path, size):
    n = int(eval(size, {"__builtins__": {}}, dict(turns)))
    assert turns["block"] == 256
    lengths = [900, 500]
    sites = sorted({(0, p) for p in range(0, 900, 7)} | {(1, p) for p in range(3, 500, 11)} | {(1, 499)})
    records = spread(n, lengths, 100 + n)
    records[-1] = rec(0, 0, 1, 450, [(M, 50)])                  # (the last lane's record lies over a site, whatever chance gave)
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths, sites, min_basequal=20)
    engine.pileup_likelihoods_damage_begin(table_of(20), noqual_quality=40)
    assert add_file(engine, tmp_path / "in.bam") == [n]
    _, _, _, _, counts = check_gld(engine.pileup_likelihoods_finish(), records, lengths, sites, 20, min_qual=20, noqual=40)
    assert counts["added"] >= 1


# ---------------------------------------------------------------------- 5. contention: ten 64-bit atomics on one strand's row
def test_two_thousand_records_over_one_site(engine, tmp_path):
    lengths = [500]
    rng = np.random.default_rng(3)
    records = [rec(0x10 * (i % 2), i % 3, 0, 100 + i % 7, [(M, 10)], "".join(rng.choice(list("ACGT"), 10)), [int(x) for x in rng.choice((2, 20, 41, 93), 10)])
               for i in range(2000)]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths, [(0, 108)], call="majority")
    engine.pileup_likelihoods_damage_begin(table_of(5))
    add_file(engine, tmp_path / "in.bam")
    sums, _, _, bases, counts = check_gld(engine.pileup_likelihoods_finish(), records, lengths, [(0, 108)], 5)
    assert counts == dict(added=2000, without_qualities=0) and bases == [2000] and np.count_nonzero(sums[0]) == 20


# ---------------------------------------------------------------------- 6. reads inside the profile, reads that reach the tail
@pytest.mark.parametrize("k", [5, 20])
def test_short_reads_and_the_tail(engine, tmp_path, k):
    """Reads of 1 .. 12 bases, shorter than K = 20 — both distances inside the profile at once — and longer than K = 5; reads of 60
    whose middle takes the tail row of either end; the records the CPU test lists (clips, insertions, D and N, no qualities)."""
    lengths = [200]
    rng = np.random.default_rng(k)
    records = [(f, lib, 0, p, c, s, q) for f, lib, _, p, c, s, q in special_records()]
    for i in range(300):
        n = 1 + i % 12 if i % 3 else 60
        records.append(rec(0x10 * (i % 2), i % 3, 0, int(rng.integers(0, 200 - n)), [(M, n)], "".join(rng.choice(list("ACGT"), n)), [int(x) for x in rng.integers(2, 42, n)]))
    sites = [(0, p) for p in range(0, 200, 2)]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths, sites)
    engine.pileup_likelihoods_damage_begin(table_of(k), noqual_quality=25)
    add_file(engine, tmp_path / "in.bam")
    _, _, best, bases, counts = check_gld(engine.pileup_likelihoods_finish(), records, lengths, sites, k, noqual=25)
    assert counts["added"] > 3000 and len(set(best)) >= 6


# ---------------------------------------------------------------------- 7. slabs; 8. state
def test_one_slab_and_many(engine, clustered):
    lengths, records, sites = clustered["lengths"], clustered["records"], clustered["sites"]
    begin(engine, lengths, sites, min_basequal=21, mask_ends=(1, 0), seed=9)
    engine.pileup_likelihoods_damage_begin(table_of(20), noqual_quality=33)
    assert len(add_file(engine, clustered["dir"] / "in.bam")) == 1
    one = engine.pileup_likelihoods_finish()
    again = engine.pileup_likelihoods_finish()              # (a finish leaves the sums as they are)
    engine.reset()                                          # (mdx_reset zeroes them)
    zero = engine.pileup_likelihoods_finish()
    assert zero[0].shape == (len(sites), 20) and not zero[0].any() and not zero[1].any() and not zero[2].any() and not zero[3].any()
    assert zero[4] == dict(added=0, without_qualities=0)
    assert len(add_file(engine, clustered["dir"] / "in.bam", 1 << 16)) >= 5
    many = engine.pileup_likelihoods_finish()
    check_gld(one, records, lengths, sites, 20, k5=1, k3=0, min_qual=21, noqual=33)
    for other in (again, many):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:4], other[:4])) and one[4] == other[4]
    assert one[4]["added"] > 10_000 and one[4]["without_qualities"] > 500


def test_the_counters_are_what_they_are_without_the_sums(engine, clustered):
    """``pileup_finish``'s five results with the damage sums present equal those without."""
    lengths, sites = clustered["lengths"], clustered["sites"]
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(sites))]
    results = []
    for with_sums in (False, True):
        begin(engine, lengths, sites, alleles, min_basequal=21, mask_ends=(3, 2), call="majority", seed=4, single_strand=True)
        if with_sums:
            engine.pileup_likelihoods_damage_begin(table_of(5))
        add_file(engine, clustered["dir"] / "in.bam", 1 << 17)
        results.append(engine.pileup_finish())
    plain, beside = results
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[:4], beside[:4])) and plain[4] == beside[4] and plain[0].any()


def test_call_order(clustered):
    from mapdamage_amd.engine import DamageEngine, MdxError
    lengths, sites = clustered["lengths"], clustered["sites"]
    pos, off = site_columns(sites, len(lengths))
    with DamageEngine(LIBS3) as other:
        other.set_reference(reference(lengths))
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_damage_begin(table_of(5))          # no pileup_begin yet
        assert error.value.code == ERR_STATE and "mdx_pileup_begin" in str(error.value)
        other.pileup_begin(pos, off)
        plain = other.pileup_info()["bytes"]
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()                           # the counters alone
        assert error.value.code == ERR_STATE
        for bad in (0, 94, -1):
            with pytest.raises(MdxError) as error:
                other.pileup_likelihoods_damage_begin(table_of(5), noqual_quality=bad)
            assert error.value.code == -1 and "1..93" in str(error.value)
        for shape in ((2, 6, 94, 3), (1, 6, 94, 9), (2, 6, 93, 9), (94, 3)):
            with pytest.raises(ValueError):
                other.pileup_likelihoods_damage_begin(np.zeros(shape, np.int64))
        for rows in (1, 256):
            with pytest.raises(MdxError) as error:
                other.pileup_likelihoods_damage_begin(np.zeros((2, rows, 94, 9), np.int64))
            assert error.value.code == -1 and "2..255" in str(error.value)
        assert other.pileup_info()["bytes"] == plain
        # one model per pileup: whichever begin comes second is refused, and the first one's sums stay
        other.pileup_likelihoods_damage_begin(table_of(5))
        with_sums = other.pileup_info()["bytes"]
        assert with_sums == plain + len(sites) * 160 + 2 * 6 * 94 * 9 * 8 + 16
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_begin()
        assert error.value.code == ERR_STATE and "one model per pileup" in str(error.value)
        assert other.pileup_likelihoods_finish()[0].shape == (len(sites), 20) and other.pileup_info()["bytes"] == with_sums
        other.pileup_likelihoods_damage_begin(table_of(20))             # again, with another K: the new table
        assert other.pileup_info()["bytes"] == plain + len(sites) * 160 + 2 * 21 * 94 * 9 * 8 + 16
        other.pileup_begin(pos, off)                                    # a second pileup_begin releases the sums
        assert other.pileup_info()["bytes"] == plain
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()
        assert error.value.code == ERR_STATE
        other.pileup_likelihoods_begin()
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_damage_begin(table_of(5))
        assert error.value.code == ERR_STATE and "one model per pileup" in str(error.value)
        assert other.pileup_likelihoods_finish()[0].shape == (len(sites), 24)
        # ... and so does a new reference
        other.pileup_begin(pos, off)
        other.pileup_likelihoods_damage_begin(table_of(5))
        other.set_reference(reference([500]))
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()
        assert error.value.code == ERR_STATE


# ---------------------------------------------------------------------- 9. the command line
def expected_damage_likelihoods(out, panel, records, n_libraries, path, profile_path, d5, d3, beagle=None, k5=0, k3=0, q=0, single_strand=False, noqual=30):
    sites, names, pairs = panel["sites"], panel["names"], panel["alleles"]
    counters, _ = PR.brute(records, n_libraries, panel["lengths"], sites, k5, k3, q)
    sums, counts = DR.brute(records, n_libraries, panel["lengths"], sites, DR.rates(d5), DR.rates(d3), k5, k3, q, noqual)
    gl, best, bases = DR.all_likelihoods(sums, counters, pairs, single_strand)
    assert GR.same_text((out / "pileup_likelihoods.tsv").read_text(), GR.likelihoods_text(names, sites, panel["ids"], pairs, gl, best, bases), GR.LIKELIHOOD_FLOATS)
    assert (out / "pileup_likelihoods_summary.tsv").read_text() == GR.summary_text(path, q, k5, k3, single_strand, noqual, bases, counts)
    if beagle is not None:
        assert GR.same_text(beagle.read_text(), GR.beagle_text(names, sites, pairs, gl, bases), GR.BEAGLE_FLOATS)
    assert (out / "pileup_damage_profile.tsv").read_text() == DR.profile_text(d5, d3)
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log and GR.log_line(noqual, bases, counts) in log and DR.log_line(profile_path, d5, d3) in log
    assert sorted(f for f in os.listdir(out) if f.startswith("pileup")) == ["pileup.tsv", "pileup_damage_profile.tsv", "pileup_likelihoods.tsv",
                                                                           "pileup_likelihoods_summary.tsv", "pileup_summary.tsv"]
    return gl, best, bases, counts


ARGS = ["--pileup-mask-ends", "1,0", "--pileup-min-basequal", "20", "--pileup-single-strand-mode", "--pileup-seed", "5"]


@pytest.fixture(scope="module")
def alone(dup_data, panel, tmp_path_factory):       # noqa: F811
    """The run with --pileup-likelihoods and without the profile: what the option must leave as it is."""
    d = tmp_path_factory.mktemp("pileup_gld_alone")
    out = run(dup_data, d / "alone", "in.bam", "--pileup-sites", panel["path"], *ARGS, "--pileup-likelihoods", "--pileup-beagle", d / "alone.beagle", "--by-reference")
    return out, d / "alone.beagle"


def test_command_line(dup_data, panel, alone, tmp_path):       # noqa: F811
    panel = dict(panel, ref=dup_data["ref"])
    alone, alone_beagle = alone
    (tmp_path / "misincorporation.txt").write_text(TEXT)
    with_option = run(dup_data, tmp_path / "with", "in.bam", "--pileup-sites", panel["path"], *ARGS, "--pileup-likelihoods", "--pileup-beagle", tmp_path / "panel.beagle",
                      "--by-reference", "--pileup-damage-profile", tmp_path / "misincorporation.txt", "--pileup-damage-positions", "5")
    gl, best, bases, counts = expected_damage_likelihoods(with_option, panel, panel["records"], 3, panel["path"], tmp_path / "misincorporation.txt", D5_K5, D3_K5,
                                                          tmp_path / "panel.beagle", 1, 0, 20, True)
    assert counts["added"] > 1000 and max(bases) >= 3 and len(set(best)) >= 4
    # every file that is no likelihood file is what it is without the option, and the likelihoods are not
    for name in ("pileup.tsv", "pileup_summary.tsv", "pileup_likelihoods_summary.tsv"):
        assert (with_option / name).read_bytes() == (alone / name).read_bytes(), name
    assert tables(with_option) == tables(alone)
    assert (with_option / "by_reference" / "groups.tsv").read_bytes() == (alone / "by_reference" / "groups.tsv").read_bytes()
    assert (with_option / "pileup_likelihoods.tsv").read_bytes() != (alone / "pileup_likelihoods.tsv").read_bytes()
    # without the option: the parent's files, no profile file, no line
    expected_likelihoods(alone, panel, panel["records"], 3, panel["path"], alone_beagle, 1, 0, 20, True)
    assert not (alone / "pileup_damage_profile.tsv").exists() and "Pileup damage profile" not in (alone / "Runtime_log.txt").read_text()
    # many slabs: the same files
    again = run(dup_data, tmp_path / "again", "in.bam", "--pileup-sites", panel["path"], *ARGS, "--pileup-likelihoods", "--pileup-damage-profile",
                tmp_path / "misincorporation.txt", "--pileup-damage-positions", "5", "--chunk-mb", "0.0625")
    for name in ("pileup_likelihoods.tsv", "pileup_likelihoods_summary.tsv", "pileup_damage_profile.tsv", "pileup.tsv"):
        assert (again / name).read_bytes() == (with_option / name).read_bytes(), name


def test_command_line_with_a_profile_without_damage(dup_data, panel, alone, tmp_path):       # noqa: F811
    """Rates of zero at every position: the files of --pileup-likelihoods alone, byte for byte."""
    alone, alone_beagle = alone
    (tmp_path / "zero.txt").write_text(DR.misincorporation_text([(0, 500)] * 30, [(0, 600)] * 30))
    zero = run(dup_data, tmp_path / "zero", "in.bam", "--pileup-sites", panel["path"], *ARGS, "--pileup-likelihoods", "--pileup-beagle", tmp_path / "zero.beagle",
               "--by-reference", "--pileup-damage-profile", tmp_path / "zero.txt")
    for name in ("pileup_likelihoods.tsv", "pileup_likelihoods_summary.tsv", "pileup.tsv", "pileup_summary.tsv"):
        assert (zero / name).read_bytes() == (alone / name).read_bytes(), name
    assert (tmp_path / "zero.beagle").read_bytes() == alone_beagle.read_bytes() and tables(zero) == tables(alone)
    assert (zero / "pileup_damage_profile.tsv").read_text().split("\n")[21] == "5p\t>20\t0\t5000\t0"


def test_command_line_with_the_run_s_own_table(dup_data, panel, alone, tmp_path):       # noqa: F811
    """The two-run workflow: the first run's misincorporation.txt is the second run's profile."""
    panel = dict(panel, ref=dup_data["ref"])
    alone, _ = alone
    profile_path = alone / "misincorporation.txt"
    d5, d3 = DR.profile(profile_path.read_text(), 10)
    assert d5[0][1] > 100 and d3[0][1] > 100
    out = run(dup_data, tmp_path / "second", "in.bam", "--pileup-sites", panel["path"], "--pileup-likelihoods", "--pileup-damage-profile", profile_path,
              "--pileup-damage-positions", "10", "--pileup-noqual-quality", "12")
    expected_damage_likelihoods(out, panel, panel["records"], 3, panel["path"], profile_path, d5, d3, noqual=12)
    assert (out / "misincorporation.txt").read_bytes() == profile_path.read_bytes()
