"""--pileup-likelihoods on the device (mapdamage_amd/csrc/mdx_pileup.hip): the sums, the ten values, the best genotype and the
bases of ``pileup_likelihoods_finish`` over the small BAM files of tests/test_gpu_pileup.py against the brute force of
tests/gl_rule.py — the hand-written table, dense sites where the add kernel's list turns, contended 64-bit atomics, record
counts around the block size, one slab and many, marked flags, the state rules, the counters' path left to itself —, and the
command line's files against the rule's.  The rule on the host, the table and the emitters: tests/test_pileup_likelihoods.py."""

import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gl_rule as GR
from tests import pileup_rule as PR
from tests.test_gpu_depth import names_of, reference
from tests.test_gpu_pileup import (DENSE_LENGTHS, DENSE_SITES, ERR_STATE, add_file, begin, check, clustered, dense_records, engine, exact_records,  # noqa: F401
                                   expected_files, panel, rule_record, site_columns, spread, turns, write_records)
from tests.test_gpu_remove_duplicates import LIBS3, dup_data      # noqa: F401  (dup_data: a fixture)
from tests.test_gpu_write_kept import DEVICE, read_bam_file, run, tables
from tests.test_pileup import HAND_LENGTHS, HAND_LIBRARIES, HAND_RECORDS, HAND_SETTINGS, HAND_SITES, rec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, P, EQ, X = range(9)
DENSE_NOQUAL = 17


def check_gl(got, records, lengths, sites, n_libraries=3, k5=0, k3=0, min_qual=0, noqual=30, alleles=None, single_strand=False):
    """What ``pileup_likelihoods_finish`` gave against the rule: every sum, every value, the best and the bases bit for bit."""
    sums, gl, best, bases, counts = got
    counters, _ = PR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual)
    want_sums, want_counts = GR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual, noqual)
    want_gl, want_best, want_bases = GR.all_likelihoods(want_sums, counters, alleles, single_strand)
    want_sums = np.array(want_sums, np.int64).reshape(-1, 24)
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
        options = dict(mode=("random", "majority", "none")[n % 3], seed=n, min_depth=1 + n % 2, single_strand=bool(n % 2))
        noqual = (30, 7, 93, 1)[n % 4]
        ref = begin(engine, HAND_LENGTHS, HAND_SITES, alleles, min_basequal=q, mask_ends=(k5, k3), call=options["mode"], seed=n,
                    min_depth=options["min_depth"], single_strand=options["single_strand"])
        plain = engine.pileup_info()["bytes"]
        engine.pileup_likelihoods_begin(noqual_quality=noqual)
        assert engine.pileup_info()["bytes"] == plain + len(HAND_SITES) * 192 + 94 * 3 * 8 + 16
        assert add_file(engine, tmp_path / "in.bam", packed=packed) == [len(HAND_RECORDS)]
        check_gl(engine.pileup_likelihoods_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, HAND_LIBRARIES, k5, k3, q, noqual, alleles, options["single_strand"])
        check(engine.pileup_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, ref, HAND_LIBRARIES, k5, k3, q, alleles=alleles, **options)
    assert engine.pileup_likelihoods_finish(with_sums=False)[0] is None


# ---------------------------------------------------------------------- 2. dense sites: the list's rounds
def test_dense_sites_with_the_whole_list(engine, turns, tmp_path):
    records = dense_records()
    write_records(tmp_path / "in.bam", records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    begin(engine, DENSE_LENGTHS, DENSE_SITES, min_basequal=20, mask_ends=(2, 1), call="majority", seed=3)
    engine.pileup_likelihoods_begin(noqual_quality=DENSE_NOQUAL)
    assert add_file(engine, tmp_path / "in.bam") == [2000]
    _, _, best, bases, counts = check_gl(engine.pileup_likelihoods_finish(), records, DENSE_LENGTHS, DENSE_SITES, k5=2, k3=1, min_qual=20, noqual=DENSE_NOQUAL)
    assert counts["added"] > 20_000 and counts["without_qualities"] > 1000 and max(bases) > 100 and len(set(best)) >= 4


@pytest.fixture(scope="module")
def small_list(tmp_path_factory):
    """A child process whose add kernel's list holds 48 pairs, as in tests/test_gpu_pileup.py, with the sums beside the counters."""
    d = tmp_path_factory.mktemp("pileup_gl_list")
    cases = {"dense": dense_records(), "exact": exact_records(48), "over": exact_records(49), "twice": exact_records(96), "alone": [rec(0x10, 0, 0, 20, [(M, 250)])]}
    for name, records in cases.items():
        write_records(d / (name + ".bam"), records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_pileup_gl_worker.py"), str(d)] + sorted(cases), cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_PILEUP_LIST="48"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    return d, cases


@pytest.mark.parametrize("case", ["dense", "exact", "over", "twice", "alone"])
def test_pairs_where_the_list_turns(small_list, case):
    d, cases = small_list
    z = np.load(d / (case + ".npz"))
    assert int(z["info"][0]) == 48
    added = dict(zip(("added", "without_qualities"), (int(x) for x in z["added"])))
    check_gl((z["sums"], z["gl"], z["best"], z["bases"], added), cases[case], DENSE_LENGTHS, DENSE_SITES, k5=2, k3=1, min_qual=20, noqual=DENSE_NOQUAL)
    counts = dict(zip(("counted", "outside", "over_a_site", "pairs"), (int(x) for x in z["counts"])))
    _, want_counts = check((z["counters"], z["refbase"], z["call"], z["depth"], counts), cases[case], DENSE_LENGTHS, DENSE_SITES, reference(DENSE_LENGTHS),
                           k5=2, k3=1, min_qual=20, mode="majority", seed=3)
    assert want_counts["pairs"] == {"exact": 48, "over": 49, "twice": 96, "alone": 250}.get(case, want_counts["pairs"])


# ---------------------------------------------------------------------- 3. contention: 64-bit atomics on one row
def test_three_thousand_records_over_one_site(engine, tmp_path):
    lengths = [500]
    rng = np.random.default_rng(3)
    records = [rec(0x10 * (i % 2), i % 3, 0, 100 + i % 7, [(M, 10)], "ACGTACGTAC", [int(x) for x in rng.choice((2, 20, 41, 93), 10)]) for i in range(3000)]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths, [(0, 108)], call="majority")
    engine.pileup_likelihoods_begin()
    add_file(engine, tmp_path / "in.bam")
    sums, _, _, bases, counts = check_gl(engine.pileup_likelihoods_finish(), records, lengths, [(0, 108)])
    assert counts == dict(added=3000, without_qualities=0) and bases == [3000] and np.count_nonzero(sums[0]) >= 21


# ---------------------------------------------------------------------- 4. record counts around the block size
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "block-1", "block", "block+1", "2*block+1"])
def test_record_counts_where_the_add_kernel_turns(engine, turns, tmp_path, size):
    n = int(eval(size, {"__builtins__": {}}, dict(turns)))
    lengths = [900, 500]
    sites = sorted({(0, p) for p in range(0, 900, 7)} | {(1, p) for p in range(3, 500, 11)} | {(1, 499)})
    records = spread(n, lengths, 100 + n)
    records[-1] = rec(0, 0, 1, 450, [(M, 50)])                  # (the last lane's record lies over a site, whatever chance gave)
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths, sites, min_basequal=20, mask_ends=(1, 1))
    engine.pileup_likelihoods_begin(noqual_quality=40)
    assert add_file(engine, tmp_path / "in.bam") == [n]
    _, _, _, _, counts = check_gl(engine.pileup_likelihoods_finish(), records, lengths, sites, k5=1, k3=1, min_qual=20, noqual=40)
    assert counts["added"] >= 1


# ---------------------------------------------------------------------- 5. slabs, flags, state
def test_one_slab_and_many(engine, clustered):
    lengths, records, sites = clustered["lengths"], clustered["records"], clustered["sites"]
    begin(engine, lengths, sites, min_basequal=21, mask_ends=(3, 0), seed=9)
    engine.pileup_likelihoods_begin(noqual_quality=33)
    assert len(add_file(engine, clustered["dir"] / "in.bam")) == 1
    one = engine.pileup_likelihoods_finish()
    again = engine.pileup_likelihoods_finish()              # (a finish leaves the sums as they are)
    engine.reset()                                          # (mdx_reset zeroes them)
    zero = engine.pileup_likelihoods_finish()
    assert not zero[0].any() and not zero[1].any() and not zero[2].any() and not zero[3].any() and zero[4] == dict(added=0, without_qualities=0)
    assert len(add_file(engine, clustered["dir"] / "in.bam", 1 << 16)) >= 5
    many = engine.pileup_likelihoods_finish()
    check_gl(one, records, lengths, sites, k5=3, k3=0, min_qual=21, noqual=33)
    for other in (again, many):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:4], other[:4])) and one[4] == other[4]
    assert one[4]["added"] > 10_000 and one[4]["without_qualities"] > 500


def test_the_flags_as_they_stand(engine, clustered):
    """0x200 and 0x400 on chosen records in front of the add: such records add nothing to the sums either."""
    lengths, records, sites = clustered["lengths"], clustered["records"][:5000], clustered["sites"]
    rng = np.random.default_rng(9)
    bits = np.zeros(len(records), np.uint16)
    bits[rng.choice(len(records), 1500, replace=False)] = 0x200
    bits[rng.choice(len(records), 1000, replace=False)] |= 0x400

    def before(stream, view, first):
        f = stream.view_flags(view)
        f |= bits[first:first + len(f)]
        stream.set_view_flags(view, f)

    path = clustered["dir"] / "first_gl.bam"
    write_records(path, records, names_of(lengths), lengths)
    begin(engine, lengths, sites)
    engine.pileup_likelihoods_begin()
    assert len(add_file(engine, path, 1 << 16, before=before)) >= 3
    marked = [(r[0] | int(b),) + r[1:] for r, b in zip(records, bits)]
    _, _, _, _, counts = check_gl(engine.pileup_likelihoods_finish(), marked, lengths, sites)
    assert 0 < counts["added"] < GR.brute(records, 3, lengths, sites)[1]["added"] * 0.7


def test_the_counters_are_what_they_are_without_the_sums(engine, clustered):
    """``pileup_finish``'s five results with the sums present equal those without."""
    lengths, sites = clustered["lengths"], clustered["sites"]
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(sites))]
    results = []
    for with_sums in (False, True):
        begin(engine, lengths, sites, alleles, min_basequal=21, mask_ends=(3, 2), call="majority", seed=4, single_strand=True)
        if with_sums:
            engine.pileup_likelihoods_begin()
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
        for call in (other.pileup_likelihoods_begin, other.pileup_likelihoods_finish):
            with pytest.raises(MdxError) as error:
                call()                                      # no pileup_begin yet
            assert error.value.code == ERR_STATE and "mdx_pileup_begin" in str(error.value)
        other.pileup_begin(pos, off)
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()               # the counters alone
        assert error.value.code == ERR_STATE
        for bad in (0, 94, -1):
            with pytest.raises(MdxError) as error:
                other.pileup_likelihoods_begin(noqual_quality=bad)
            assert error.value.code == -1 and "1..93" in str(error.value)
        with pytest.raises(ValueError):
            other.pileup_likelihoods_begin(np.zeros((93, 3), np.int64))
        other.pileup_likelihoods_begin()
        with_sums = other.pileup_info()["bytes"]
        assert other.pileup_likelihoods_finish()[1].shape == (len(sites), 10)
        # a second pileup_begin releases the sums
        other.pileup_begin(pos, off)
        assert other.pileup_info()["bytes"] == with_sums - len(sites) * 192 - 94 * 3 * 8 - 16
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()
        assert error.value.code == ERR_STATE
        # ... and so does a new reference
        other.pileup_likelihoods_begin()
        other.set_reference(reference([500]))
        with pytest.raises(MdxError) as error:
            other.pileup_likelihoods_finish()
        assert error.value.code == ERR_STATE


# ---------------------------------------------------------------------- 6. the command line
def expected_likelihoods(out, panel, records, n_libraries, path, beagle=None, k5=0, k3=0, q=0, single_strand=False, noqual=30, alleles=True):
    sites, names = panel["sites"], panel["names"]
    pairs = panel["alleles"] if alleles else None
    counters, _ = PR.brute(records, n_libraries, panel["lengths"], sites, k5, k3, q)
    sums, counts = GR.brute(records, n_libraries, panel["lengths"], sites, k5, k3, q, noqual)
    gl, best, bases = GR.all_likelihoods(sums, counters, pairs, single_strand)
    assert GR.same_text((out / "pileup_likelihoods.tsv").read_text(), GR.likelihoods_text(names, sites, panel["ids"] if alleles else None, pairs, gl, best, bases),
                        GR.LIKELIHOOD_FLOATS)
    assert (out / "pileup_likelihoods_summary.tsv").read_text() == GR.summary_text(path, q, k5, k3, single_strand, noqual, bases, counts)
    if beagle is not None:
        text = gzip.decompress(beagle.read_bytes()).decode() if str(beagle).endswith(".gz") else beagle.read_text()
        assert GR.same_text(text, GR.beagle_text(names, sites, pairs, gl, bases), GR.BEAGLE_FLOATS)
        assert all(abs(sum(float(x) for x in line.split("\t")[3:]) - 1) <= 2e-6 for line in text.split("\n")[1:-1])
        assert [f for f in os.listdir(beagle.parent) if f.startswith(beagle.name) and f != beagle.name] == []
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log and GR.log_line(noqual, bases, counts) in log
    assert sorted(f for f in os.listdir(out) if f.startswith("pileup")) == ["pileup.tsv", "pileup_likelihoods.tsv", "pileup_likelihoods_summary.tsv",
                                                                           "pileup_summary.tsv"]
    return gl, best, bases, counts


def test_command_line(dup_data, panel, tmp_path):
    panel = dict(panel, ref=dup_data["ref"])
    args = ["--pileup-sites", panel["path"], "--pileup-mask-ends", "2,1", "--pileup-min-basequal", "20", "--pileup-single-strand-mode", "--pileup-seed", "5"]
    with_option = run(dup_data, tmp_path / "with", "in.bam", *args, "--pileup-likelihoods", "--pileup-beagle", tmp_path / "panel.beagle", "--by-reference")
    without = run(dup_data, tmp_path / "without", "in.bam", *args, "--by-reference")
    gl, best, bases, counts = expected_likelihoods(with_option, panel, panel["records"], 3, panel["path"], tmp_path / "panel.beagle", 2, 1, 20, True)
    assert counts["added"] > 1000 and max(bases) >= 3 and len(set(best)) >= 4
    # every other file is what it is without the option, the pileup's two among them; without it neither file nor line
    expected_files(without, panel, panel["records"], 3, panel["path"], 2, 1, 20, seed=5, single_strand=True)
    for name in ("pileup.tsv", "pileup_summary.tsv"):
        assert (with_option / name).read_bytes() == (without / name).read_bytes(), name
    assert tables(with_option) == tables(without)
    assert (with_option / "by_reference" / "groups.tsv").read_bytes() == (without / "by_reference" / "groups.tsv").read_bytes()
    assert not (without / "pileup_likelihoods.tsv").exists() and not (without / "pileup_likelihoods_summary.tsv").exists()
    assert "Pileup likelihoods" not in (without / "Runtime_log.txt").read_text()      # (the log's first line names the command, this file in it)
    # a .gz path, read back with gzip: the same text; many slabs and another noqual quality
    again = run(dup_data, tmp_path / "again", "in.bam", *args, "--pileup-likelihoods", "--pileup-beagle", tmp_path / "panel.beagle.gz", "--chunk-mb", "0.0625")
    assert gzip.decompress((tmp_path / "panel.beagle.gz").read_bytes()) == (tmp_path / "panel.beagle").read_bytes()
    assert (again / "pileup_likelihoods.tsv").read_bytes() == (with_option / "pileup_likelihoods.tsv").read_bytes()
    expected_likelihoods(again, panel, panel["records"], 3, panel["path"], tmp_path / "panel.beagle.gz", 2, 1, 20, True)


def test_command_line_without_alleles(dup_data, panel, tmp_path):
    panel = dict(panel, ref=dup_data["ref"])
    out = run(dup_data, tmp_path / "plain", "in.bam", "--pileup-sites", panel["plain"], "--pileup-likelihoods", "--pileup-noqual-quality", "12", "--pileup-call", "none")
    _, best, bases, _ = expected_likelihoods(out, panel, panel["records"], 3, panel["plain"], noqual=12, alleles=False)
    lines = (out / "pileup_likelihoods.tsv").read_text().split("\n")[1:-1]
    assert all(line.split("\t")[2:5] == [".", ".", "."] for line in lines) and [line.split("\t")[-1] == "." for line in lines] == [n == 0 for n in bases]


def test_command_line_beside_the_pipeline(dup_data, panel, tmp_path):
    """Beside --remove-duplicates --write-kept the likelihoods are the brute force over the records of the written file."""
    panel = dict(panel, ref=dup_data["ref"])
    args = ["--remove-duplicates", "--min-mapq", "25", "--write-kept"]
    with_option = run(dup_data, tmp_path / "with", "in.bam", *args, tmp_path / "kept.bam", "--pileup-sites", panel["path"], "--pileup-likelihoods")
    without = run(dup_data, tmp_path / "without", "in.bam", *args, tmp_path / "kept0.bam", "--pileup-sites", panel["path"])
    written = [rule_record(raw, 0) for raw in read_bam_file(tmp_path / "kept.bam")[1]]
    assert len(written) > 500
    _, _, _, counts = expected_likelihoods(with_option, panel, written, 1, panel["path"])
    assert counts["added"] > 500
    assert tables(with_option) == tables(without) and (tmp_path / "kept.bam").read_bytes() == (tmp_path / "kept0.bam").read_bytes()
    for name in ("pileup.tsv", "pileup_summary.tsv", "duplicates.tsv", "duplicates_histogram.tsv"):
        assert (with_option / name).read_bytes() == (without / name).read_bytes(), name
