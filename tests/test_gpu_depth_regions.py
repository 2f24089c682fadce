"""--depth-regions on the device (``depth_regions_kernel`` of mapdamage_amd/csrc/mdx_depth.hip, ``mdx_depth_regions``): the three
arrays of ``DamageEngine.depth_regions`` — per interval, per group, the groups' histograms — integer-exact against the brute force
of tests/depth_regions_rule.py, with intervals placed where the pass turns (a lane's 16 elements, a wavefront's 1024, a tile's
4096, a sequence's end, the scan's round), and the command line's four files against the same brute force over the file the run
wrote.  The emitters and the argument errors: tests/test_depth_regions.py."""

import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import fasta
from mapdamage_amd import tables as T
from mapdamage_amd.batch import Reference
from tests import depth_regions_rule as RR
from tests import depth_rule as PR
from tests.test_gpu_depth import LIBS3, M, D, add_file, names_of, reference, spread, write_records
from tests.test_gpu_remove_duplicates import dup_data      # noqa: F401  (a fixture)
from tests.test_gpu_write_kept import DEVICE, read_bam_file, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -3
FOUR = ("coverage.tsv", "depth_histogram.tsv", "depth_thresholds.tsv", "regions_depth.tsv")
ABC = ["a", "b", "*"]


def columns(regions, n_contig):
    """``regions``: (tid, start, end, group), sorted -> iv_off, iv_start, iv_end, iv_group."""
    assert regions == sorted(regions)
    off = np.zeros(n_contig + 1, np.int64)
    for t, _, _, _ in regions:
        off[t + 1:] += 1
    return (off,) + tuple(np.array([r[q] for r in regions], np.int32) for q in (1, 2, 3))


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS3, groups=ABC) as eng:
        yield eng


@pytest.fixture(scope="module")
def turns(engine):
    """The elements of a lane, a wavefront and a tile of the finish, from ``mdx_depth_info``: a block of as many lanes as the add
    kernel's takes records, a tile of them."""
    engine.set_reference(reference([100]))
    engine.depth_begin()
    info = engine.depth_info()
    tile, lane = info["tile"], info["tile"] // info["block_records"]
    assert lane * info["block_records"] == tile and 4 <= lane <= 64
    return dict(lane=lane, wave=64 * lane, tile=tile)


def begin(eng, ref, regions):
    """``ref`` resident (a list of lengths: random bases), the intervals set, a fresh accumulator.  -> the columns."""
    lengths = ref if isinstance(ref, list) else ref.lengths
    eng.set_reference(reference(ref) if isinstance(ref, list) else ref)
    cols = columns(regions, len(lengths))
    eng.set_strata_regions(*cols)
    eng.depth_begin()
    return cols


def same(got, want):
    return all(a.dtype == b.dtype == np.uint64 and a.shape == b.shape and (a == b).all() for a, b in zip(got, want))


def check(eng, records, lengths, cols, n_groups=3, n_libraries=3):
    base = PR.brute(records, n_libraries, lengths)
    want = RR.brute(base["depth"], *cols, n_groups)
    got = eng.depth_regions()
    for a, b, what in zip(got, want, ("per interval", "per group", "histograms")):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert (a == b).all(), (what, np.argwhere(a != b)[:8].tolist(), a[a != b][:8].tolist(), b[a != b][:8].tolist())
    # what holds between the two finishes, whatever the records
    per_contig, hist, _ = eng.depth_finish()
    per_interval, per_group, group_hist = got
    assert (per_contig == base["per_contig"]).all() and (hist == base["hist"]).all()
    assert (group_hist.sum(axis=0) == hist).all()
    assert (group_hist.sum(axis=1) == per_group[:, 0]).all() and int(per_group[:, 0].sum()) == sum(lengths)
    assert int(per_group[:, 1].sum()) == int(per_contig[:, 1].sum()) and int(per_group[:, 2].sum()) == int(per_contig[:, 2].sum())
    assert int(per_group[:, 3].max()) == (int(per_contig[:, 3].max()) if len(per_contig) else 0)
    return dict(got=got, depth=base["depth"], base=base)


def case(eng, tmp_path, lengths, regions, records, **kw):
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    cols = begin(eng, lengths, regions)
    add_file(eng, tmp_path / "in.bam")
    return check(eng, records, lengths, cols, **kw)


# ---------------------------------------------------------------------- 1. lanes, wavefronts, tiles
def test_intervals_against_lanes_wavefronts_and_tiles(engine, turns, tmp_path):
    lane, wave, tile = turns["lane"], turns["wave"], turns["tile"]
    lengths = [4 * tile + 100]
    regions = [(0, 3, 9, 0),                                       # inside one lane's elements
               (0, lane - 2, lane + 5, 1),                         # across a lane's edge
               (0, wave - 3, wave + 3, 0),                         # across a wavefront's
               (0, tile - 5, tile + 5, 1),                         # across a tile's
               (0, 2 * tile - 100, 3 * tile + 100, 0)]             # a whole tile and parts of both neighbours; the last tile has none
    out = case(engine, tmp_path, lengths, regions, spread(3000, lengths, 21) + [(0, 0, 0, 0, [(M, 20)]), (0, 1, 0, wave - 10, [(M, 30)])])
    per_interval = out["got"][0]
    assert per_interval[4, 1] > tile and (per_interval[:, 0] > 0).all()


# ---------------------------------------------------------------------- 2. single bases, abutting groups
def test_single_bases_and_abutting_groups(engine, turns, tmp_path):
    lane, tile = turns["lane"], turns["tile"]
    lengths = [tile + 500]
    regions = ([(0, 2 * lane + j, 2 * lane + j + 1, j % 2) for j in range(lane)]                      # a lane's elements, a base each
               + [(0, 4 * lane + 10, 5 * lane, 0), (0, 5 * lane, 5 * lane + 10, 1)]                   # abutting at a lane's edge
               + [(0, tile - 20, tile, 1), (0, tile, tile + 20, 0)])                                  # ... at a tile's
    records = spread(2000, lengths, 22) + [(0, 0, 0, 2 * lane + 3, [(M, 5)]), (0, 1, 0, 2 * lane + 4, [(M, 1)]), (0, 2, 0, tile - 3, [(M, 6)])]
    out = case(engine, tmp_path, lengths, regions, records)
    per_interval = out["got"][0]
    # a single base: covered <= 1, min == max == aligned
    assert (per_interval[:lane, 0] <= 1).all() and (per_interval[:lane, 2] == per_interval[:lane, 3]).all()
    assert (per_interval[:lane, 1] == per_interval[:lane, 3]).all() and per_interval[4, 2] >= 2


# ---------------------------------------------------------------------- 3. sequences
@pytest.mark.parametrize("whole_tiles", [True, False])
def test_sequence_boundaries(engine, turns, tmp_path, whole_tiles):
    """Eight sequences: the first ends in the middle of a tile, the second on a tile's edge, then one of a single base that is an
    interval, two empty ones (names the FASTA lacks), two without intervals, and a last one whose last interval ends at G."""
    tile = turns["tile"]
    last = tile - 701 - (0 if whole_tiles else 77)
    lengths = [1000, tile - 1000, 1, 0, 0, 500, 200, last]
    assert (sum(lengths) % tile == 0) == whole_tiles
    names = names_of(lengths)
    full = reference(lengths)
    keep = [t for t, n in enumerate(lengths) if n]
    fasta.write_fasta(tmp_path / "ref.fa", Reference([names[t] for t in keep], [full.seqs[t] for t in keep]))
    ref = fasta.FastaOnDisk(tmp_path / "ref.fa", names, lengths, missing_ok=True)
    regions = [(0, 900, 1000, 0), (1, 0, 50, 1),                   # one ends with its sequence, the next begins the next one: mid-tile
               (1, tile - 1100, tile - 1000, 0), (2, 0, 1, 1),     # the same on a tile's edge; the sequence of one base
               (7, 0, 10, 0), (7, last - 30, last, 1)]             # ... and the last interval ends at G
    records = spread(1500, lengths, 23) + [
        (0, 0, 0, 990, [(M, 10)]), (0, 1, 1, 0, [(M, 7)]), (0, 0, 1, tile - 1006, [(M, 6)]), (0, 2, 2, 0, [(M, 1)]), (0, 0, 2, 0, [(M, 1)]),
        (0, 0, 7, 0, [(M, 3)]), (0, 1, 7, last - 5, [(M, 5)]), (0, 0, 3, 0, [(M, 1)])]
    write_records(tmp_path / "in.bam", records, names, lengths)
    engine.set_reference(ref)
    assert ref.lengths == lengths
    cols = columns(regions, len(lengths))
    engine.set_strata_regions(*cols)
    engine.depth_begin()
    add_file(engine, tmp_path / "in.bam")
    out = check(engine, records, lengths, cols)
    per_interval = out["got"][0]
    assert per_interval[3].tolist() == [1, 2, 2, 2] and per_interval[5, 3] >= 1 and per_interval[0, 3] >= 1 and per_interval[2, 3] >= 1


# ---------------------------------------------------------------------- 4. nothing, everything, very deep
def test_uncovered_covered_and_deeper_than_the_last_bin(engine, tmp_path):
    lengths = [3000, 2000]
    regions = [(0, 100, 200, 0),                                   # no read at all
               (0, 500, 530, 1),                                   # twenty thousand deep, every base
               (0, 540, 560, 0),                                   # ... the deletion's two bases and the read's end inside
               (0, 1010, 1040, 1)]                                 # three deep, every base
    records = ([(0, 1, 0, 500, [(M, 30), (D, 2), (M, 20)])] * 20_000 + [(0, 0, 0, 1000, [(M, 50)])] * 3
               + [(0, 2, 1, 100, [(M, 50)])] * 20_000 + [(0, 0, 1, 120, [(M, 10)])])          # off target: 20 001 deep
    out = case(engine, tmp_path, lengths, regions, records)
    per_interval, per_group, group_hist = out["got"]
    assert per_interval.tolist() == [[0, 0, 0, 0], [30, 600_000, 20_000, 20_000], [12, 240_000, 0, 20_000], [30, 90, 3, 3]]
    assert per_group[2].tolist() == [5000 - 180, 8 + 20 + 50, 8 * 20_000 + 20 * 3 + 50 * 20_000 + 10, 20_001]
    assert group_hist[1, 1023] == 30 and group_hist[0, 1023] == 12 and group_hist[2, 1023] == 58 and group_hist[0, 0] == 108


# ---------------------------------------------------------------------- 5. groups
def test_one_named_group_and_no_interval_at_all(turns, tmp_path):
    from mapdamage_amd.engine import DamageEngine
    tile = turns["tile"]
    lengths = [tile + 300, 700]
    records = spread(2000, lengths, 25)
    with DamageEngine(LIBS3, groups=["regions", "*"]) as eng:
        out = case(eng, tmp_path, lengths, [(0, 10, 90, 0), (0, tile - 40, tile + 40, 0), (1, 600, 700, 0)], records, n_groups=2)
        assert out["got"][1][0, 0] == 260
        # no interval: everything is the rest, and its row is the whole reference's
        cols = begin(eng, lengths, [])
        add_file(eng, tmp_path / "in.bam")
        out = check(eng, records, lengths, cols, n_groups=2)
        per_interval, per_group, group_hist = out["got"]
        assert per_interval.shape == (0, 4) and per_group[0].tolist() == [0, 0, 0, 0] and not group_hist[0].any()
        assert (group_hist[1] == out["base"]["hist"]).all()


def test_more_groups_than_any_lds_table_holds(turns, tmp_path):
    """300 groups, round-robin over 600 intervals of 1 to 12 bases, some abutting: 300 histograms are 2.4 MB."""
    from mapdamage_amd.engine import DamageEngine
    tile = turns["tile"]
    lengths = [2 * tile + 50]
    rng = np.random.default_rng(26)
    regions, at = [], 5
    for k in range(600):
        at += int(rng.integers(0, 9))
        width = int(rng.integers(1, 13))
        regions.append((0, at, at + width, k % 300))
        at += width
    assert tile < at <= lengths[0]
    with DamageEngine([("s", "l")], lgd_max=1024, groups=["g%d" % g for g in range(300)] + ["*"]) as eng:
        out = case(eng, tmp_path, lengths, regions, spread(3000, lengths, 27, n_libraries=1), n_groups=301, n_libraries=1)
    per_group = out["got"][1]
    assert (per_group[:300, 0] >= 2).all() and (per_group[:300, 2] > 0).all()


# ---------------------------------------------------------------------- 6. the scan's round
def test_intervals_across_the_scans_round(turns, tmp_path):
    """A child process whose scan takes four tiles a round: intervals across the element where the second and the third round begin."""
    tile = turns["tile"]
    lengths = [9 * tile + 3]
    regions = [(0, 100, 200, 0), (0, 4 * tile - 50, 4 * tile + 50, 1), (0, 4 * tile + 50, 4 * tile + 60, 0), (0, 7 * tile, 8 * tile + 9, 1),
               (0, 9 * tile - 2, 9 * tile + 3, 0)]
    records = spread(2500, lengths, 28) + [(0, 1, 0, lengths[0] - 1, [(M, 1)]), (0, 2, 0, 4 * tile - 10, [(M, 30)])]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    cols = columns(regions, 1)
    np.savez(tmp_path / "regions.npz", iv_off=cols[0], iv_start=cols[1], iv_end=cols[2], iv_group=cols[3])
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_depth_regions_worker.py"), str(tmp_path), str(lengths[0])],
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_DEPTH_ROUND="4"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    z = np.load(tmp_path / "out.npz")
    assert int(z["info"][2]) == 4 and int(z["info"][1]) == tile
    base = PR.brute(records, 3, lengths)
    want = RR.brute(base["depth"], *cols, 3)
    assert same((z["per_interval"], z["per_group"], z["group_hist"]), want)
    assert (z["hist"] == base["hist"]).all() and (z["group_hist"].sum(axis=0) == z["hist"]).all()
    assert z["per_interval"][3, 1] > 0 and z["per_interval"][4, 3] >= 1


# ---------------------------------------------------------------------- 7. slabs, order, state
@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    lengths = [30_000, 1, 12_000]
    records = spread(8000, lengths, 41)
    d = tmp_path_factory.mktemp("depth_regions_clustered")
    write_records(d / "in.bam", records, names_of(lengths), lengths)
    write_records(d / "reversed.bam", records[::-1], names_of(lengths), lengths)
    write_records(d / "a.bam", records[:700], names_of(lengths), lengths)
    write_records(d / "b.bam", records[700:1500], names_of(lengths), lengths)
    regions = [(0, 0, 120, 0), (0, 4000, 4200, 1), (0, 4200, 9000, 0), (0, 29_990, 30_000, 1), (1, 0, 1, 0), (2, 5, 6, 1), (2, 11_000, 12_000, 0)]
    return dict(dir=d, records=records, lengths=lengths, regions=regions)


def test_one_slab_and_many_and_the_reversed_file(engine, clustered):
    lengths, records, d = clustered["lengths"], clustered["records"], clustered["dir"]
    cols = begin(engine, lengths, clustered["regions"])
    assert len(add_file(engine, d / "in.bam")) == 1
    one = check(engine, records, lengths, cols)["got"]
    assert same(engine.depth_regions(), one)                       # (the call leaves the accumulator as it is)
    engine.depth_begin()
    assert len(add_file(engine, d / "in.bam", 1 << 16)) >= 4
    assert same(engine.depth_regions(), one)
    engine.reset()
    add_file(engine, d / "reversed.bam", 1 << 16)
    assert same(engine.depth_regions(), one)


def test_a_call_between_two_adds_and_reset(engine, clustered):
    lengths, records, d = clustered["lengths"], clustered["records"], clustered["dir"]
    cols = begin(engine, lengths, clustered["regions"])
    add_file(engine, d / "a.bam")
    check(engine, records[:700], lengths, cols)
    held = engine.depth_info()["bytes"]
    add_file(engine, d / "b.bam")
    check(engine, records[:1500], lengths, cols)
    engine.reset()
    # (mdx_reset releases what the call laid out: the accumulator's own bytes are what is left)
    assert engine.depth_info()["bytes"] == held - (len(clustered["regions"]) * (16 + 32) + 3 * 1024 * 8 + 32)
    zero = check(engine, [], lengths, cols)["got"]
    assert not zero[0].any() and zero[1][:, 1:].sum() == 0 and zero[2][:, 0].sum() == sum(lengths)
    assert engine.depth_info()["bytes"] == held
    add_file(engine, d / "b.bam")
    check(engine, records[700:1500], lengths, cols)


def test_call_order_and_an_interval_beyond_its_sequence(clustered):
    from mapdamage_amd.engine import DamageEngine, MdxError
    lengths, records, d = clustered["lengths"], clustered["records"], clustered["dir"]
    with DamageEngine(LIBS3) as plain:
        plain.set_reference(reference(lengths))
        plain.depth_begin()
        with pytest.raises(MdxError) as error:
            plain.depth_regions()                                  # no region strata
        assert error.value.code == ERR_STATE and "mdx_set_strata_regions" in str(error.value)
    with DamageEngine(LIBS3, groups=ABC) as eng:
        eng.set_reference(reference(lengths))
        good = columns(clustered["regions"], 3)
        eng.set_strata_regions(*good)
        with pytest.raises(MdxError) as error:
            eng.depth_regions()                                    # no accumulator
        assert error.value.code == ERR_STATE and "mdx_depth_begin" in str(error.value)
        eng.depth_begin()
        add_file(eng, d / "a.bam")
        # an interval that ends one base behind its sequence — the one of a single base —, which the setter cannot know
        bad = columns([(0, 0, 120, 0), (1, 0, 2, 1), (2, 5, 6, 1)], 3)
        eng.set_strata_regions(*bad)
        for _ in range(2):
            with pytest.raises(MdxError) as error:
                eng.depth_regions()
            assert error.value.code == ERR_ARG and "interval 1 (sequence 1, [0, 2))" in str(error.value) and "1 bases" in str(error.value)
        # the context goes on: the depth is there, and good intervals part it
        base = PR.brute(records[:700], 3, lengths)
        per_contig, hist, _ = eng.depth_finish()
        assert (per_contig == base["per_contig"]).all() and (hist == base["hist"]).all()
        eng.set_strata_regions(*good)
        check(eng, records[:700], lengths, good)
        # a new reference releases the accumulator, and with it what the call held
        eng.set_reference(reference(lengths))
        with pytest.raises(MdxError) as error:
            eng.depth_regions()
        assert error.value.code == ERR_STATE


# ---------------------------------------------------------------------- 8. the command line
def written_records(path):
    out = []
    for r in read_bam_file(path)[1]:
        tid, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", r, 4)
        words = struct.unpack_from("<%dI" % n_cigar, r, 36 + l_name)
        out.append((flag, 0, tid, pos, [(w & 15, w >> 4) for w in words]))
    return out


def bed_for(ref, path):
    """Three named groups over genome5: overlapping and abutting regions of one group (merged), abutting regions of two (apart),
    a region that ends with its sequence, a sequence without regions."""
    names, lengths = list(ref.names), [int(x) for x in ref.lengths]
    assert len(names) >= 3 and min(lengths[:3]) >= 1000
    lines = [(names[0], 100, 400, "baits"), (names[0], 350, 600, "baits"), (names[0], 600, 700, "baits"), (names[0], 700, 900, "other"),
             (names[1], 0, 1, "single"), (names[1], lengths[1] - 250, lengths[1], "other"), (names[2], 500, 520, "baits"),
             (names[2], 10, 20, "single")]
    path.write_text("".join("%s\t%d\t%d\t%s\n" % line for line in lines))
    return path


def expected_four(out, ref, bed, records, thresholds=(1, 5, 10, 20)):
    names, lengths = list(ref.names), [int(x) for x in ref.lengths]
    groups, *cols = T.parse_regions(bed.read_text(), names, lengths, named=True)
    assert groups == ["baits", "other", "single", "*"] and len(cols[1]) == 6
    base = PR.brute(records, 1, lengths)
    per_interval, per_group, group_hist = RR.brute(base["depth"], *cols, len(groups))
    d = out / "by_region"
    assert (d / "coverage.tsv").read_text() == RR.coverage_text(groups, cols[3], per_group)
    assert (d / "depth_histogram.tsv").read_text() == RR.histogram_text(groups, group_hist)
    assert (d / "depth_thresholds.tsv").read_text() == RR.thresholds_text(groups, per_group, group_hist, list(thresholds))
    assert (d / "regions_depth.tsv").read_text() == RR.regions_depth_text(names, groups, *cols, per_interval)
    assert not [p for p in os.listdir(d) if p.endswith(".tmp")]
    # the Regions and Bases of groups.tsv; a group's histogram lines sum to its bases
    rows = [line.split("\t") for line in (d / "groups.tsv").read_text().splitlines()[1:]]
    assert [line.split("\t")[:4] for line in (d / "coverage.tsv").read_text().splitlines()[1:]] == [r[:4] for r in rows]
    for g, r in enumerate(rows):
        assert sum(int(x.split("\t")[3]) for x in (d / "depth_histogram.tsv").read_text().splitlines()[1:] if x.startswith("%d\t" % g)) == int(r[3])
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    named = per_group[:-1].sum(axis=0)
    assert "Depth on target: %d of %d target bases covered (" % (named[1], named[0]) in log
    assert per_group[:-1, 2].sum() > 0 and per_group[-1, 2] > 0
    return per_group


def tree(folder):
    return {os.path.relpath(os.path.join(r, f), folder): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(folder) for f in fs}


@pytest.mark.parametrize("route", ["file", "pipe"])
def test_command_line(dup_data, tmp_path, route):
    ref = dup_data["ref"]
    bed = bed_for(ref, tmp_path / "targets.bed")
    kept = tmp_path / "kept.bam"
    out = run(dup_data, tmp_path / "with", "in.bam", "--region-groups", bed, "--depth", "--depth-regions", "--write-kept", kept, route=route)
    records = written_records(kept)
    assert len(records) > 500
    expected_four(out, ref, bed, records)
    if route == "file":
        # everything else the run writes is what it writes without the option, which leaves none of the four
        # (the same path again: write_kept.tsv names it)
        written = kept.read_bytes()
        without = run(dup_data, tmp_path / "without", "in.bam", "--region-groups", bed, "--depth", "--write-kept", kept)
        a, b = tree(out), tree(without)
        a.pop("Runtime_log.txt"), b.pop("Runtime_log.txt")
        four = {os.path.join("by_region", f) for f in FOUR}
        assert set(a) - set(b) == four and set(b) <= set(a) and len(b) > 6
        assert [k for k in sorted(b) if a[k] != b[k]] == []
        assert kept.read_bytes() == written
        assert "Depth on target" not in (without / "Runtime_log.txt").read_text()
        strip = lambda text: [line.split("\t", 1)[-1] for line in text.splitlines() if "Depth on target" not in line and "seconds" not in line]
        assert len(strip((out / "Runtime_log.txt").read_text())) == len(strip((without / "Runtime_log.txt").read_text()))


def test_command_line_behind_the_duplicates(dup_data, tmp_path):
    ref = dup_data["ref"]
    bed = bed_for(ref, tmp_path / "targets.bed")
    kept = tmp_path / "kept.bam"
    out = run(dup_data, tmp_path / "out", "in.bam", "--region-groups", bed, "--remove-duplicates", "--depth", "--depth-regions",
              "--depth-thresholds", "2,3,40", "--write-kept", kept)
    records = written_records(kept)
    plain = run(dup_data, tmp_path / "plain", "in.bam", "--region-groups", bed, "--depth", "--depth-regions", "--only-regions")
    per_group = expected_four(out, ref, bed, records, thresholds=(2, 3, 40))
    # (fewer aligned bases than with the duplicates in)
    first = lambda folder: int((folder / "by_region" / "coverage.tsv").read_text().splitlines()[1].split("\t")[6])
    assert first(out) == int(per_group[0, 2]) < first(plain)
