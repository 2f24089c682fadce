"""--depth on the device (mapdamage_amd/csrc/mdx_depth.hip): ``depth_fetch`` over every sequence, the three outputs of
``depth_finish`` and ``depth_runs`` of small BAM files against the brute force of tests/depth_rule.py — at the sizes where the
kernels turn, across sequence boundaries, under contention, in one slab and in many, behind marked flags —, and the command
line's files against the rule's.  The rule on the host and the emitters: tests/test_depth.py."""

import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import fasta, sam
from mapdamage_amd.batch import Reference
from tests import depth_rule as PR
from tests import dup_rule as DR
from tests.test_depth import HAND, HAND_LENGTHS, HAND_LIBRARIES
from tests.test_gpu_remove_duplicates import LIBS3, RG3, _mapq, dup_data      # noqa: F401  (dup_data: a fixture)
from tests.test_gpu_write_kept import DEVICE, FILES, read_bam_file, run, tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
ERR_STATE = -3


# ---------------------------------------------------------------------- files, references, results
def raw_header(names, lengths):
    text = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % nl for nl in zip(names, lengths))
            + "".join("@RG\tID:%s\tSM:%s\tLB:%s\n" % (rg, s, l) for rg, (s, l) in zip(RG3, LIBS3)))
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(names))
    for name, length in zip(names, lengths):
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out


def write_records(path, records, names, lengths):
    """``records``: (flag, lib, tid, pos, cigar) in file order; a library beyond the three gets a read group nobody knows."""
    bodies = [DR.body(f, t, p, c, rg=RG3[lib] if lib < 3 else "zz", salt=i) for i, (f, lib, t, p, c) in enumerate(records)]
    sam.write_bam_raw(str(path), raw_header(names, lengths), bodies)


def names_of(lengths):
    return ["seq%d" % t for t in range(len(lengths))]


def reference(lengths, seed=5):
    rng = np.random.default_rng(seed)
    return Reference(names_of(lengths), [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes() for n in lengths])


def add_file(eng, path, chunk_bytes=256 << 20, before=None):
    """Every slab of the file through ``depth_add``; ``before(stream, view, first record)`` runs in front of each add.  -> the slabs' sizes."""
    slabs = []
    with sam.GpuBamStream(eng, str(path), readgroups=[(rg, i) for i, rg in enumerate(RG3)], chunk_bytes=chunk_bytes) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                break
            if before is not None:
                before(stream, view, sum(slabs))
            eng.depth_add(view)
            slabs.append(int(view.n_reads))
        eng.sync()
    return slabs


def collect(eng, lengths):
    """All three views of the accumulator: every base through ``depth_fetch``, ``depth_finish``, ``depth_runs``."""
    per_contig, hist, counts = eng.depth_finish()
    return dict(fetch=[eng.depth_fetch(t, 0, n) for t, n in enumerate(lengths)], per_contig=per_contig, hist=hist, counts=counts,
                runs=eng.depth_runs())


def check(got, records, lengths, n_libraries=3):
    want = PR.brute(records, n_libraries, lengths)
    for t, (a, b) in enumerate(zip(got["fetch"], want["depth"])):
        assert len(a) == len(b) and (a.astype(np.int64) == b).all(), (t, np.flatnonzero(a.astype(np.int64) != b)[:10])
    assert (got["per_contig"] == want["per_contig"]).all(), (got["per_contig"], want["per_contig"])
    assert (got["hist"] == want["hist"]).all(), np.flatnonzero(got["hist"] != want["hist"])[:10]
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    for a, b, what in zip(got["runs"], want["runs"], ("tid", "start", "end", "depth")):
        assert a.dtype == b.dtype and len(a) == len(b) and (a == b).all(), what
    # what holds between them, whatever the records
    assert int(got["hist"].sum()) == sum(lengths)
    tid, start, end, depth = got["runs"]
    assert int(((end - start) * depth.astype(np.int64)).sum()) == int(got["per_contig"][:, 2].sum())
    assert int((end - start).sum()) == int(got["per_contig"][:, 1].sum())
    return want


def spread(n, lengths, seed, n_libraries=3):
    """``n`` records over the sequences, a few shapes of CIGAR, some at either end of their sequence, one of twenty not counted."""
    rng = np.random.default_rng(seed)
    placed = [t for t, length in enumerate(lengths) if length >= 80]
    out = []
    for i in range(n):
        t = placed[int(rng.integers(0, len(placed)))]
        cigar = [[(M, 50)], [(M, 20), (D, 5), (M, 20)], [(S, 5), (M, 30), (I, 2), (EQ, 30)], [(M, 10), (N, 30), (X, 1), (M, 9)], [(M, 1)]][int(rng.integers(0, 5))]
        span = sum(ln for op, ln in cigar if op in (M, D, N, EQ, X))
        where = rng.random()
        pos = 0 if where < 0.05 else lengths[t] - span if where < 0.1 else int(rng.integers(0, lengths[t] - span + 1))
        flag = int(rng.choice((0, 0x10))) | (int(rng.choice((0x4, 0x400, 0x200, 0x100))) if rng.random() < 0.05 else 0)
        out.append((flag, i % n_libraries, t, pos, cigar))
    return out


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS3) as eng:
        yield eng


def begin(eng, lengths):
    """The reference of these lengths resident, a fresh accumulator over it (a new reference releases the old one's)."""
    eng.set_reference(reference(lengths))
    eng.depth_begin()


@pytest.fixture(scope="module")
def turns(engine):
    """The records a block of the add kernel takes, the elements of a tile and the tiles a round of the scan takes, as the
    library tells them (``mdx_depth_info``)."""
    begin(engine, [100])
    info = engine.depth_info()
    assert 64 <= info["block_records"] <= 1024 and 256 <= info["tile"] <= 1 << 16 and 4 < info["round_tiles"] <= 1 << 16
    # (diff[G + 1] in whole tiles, 4 bytes an element)
    assert info["bytes"] >= 4 * info["tile"]
    return dict(block=info["block_records"], tile=info["tile"], round=info["round_tiles"])


def sized(turns, size):
    return int(eval(size, {"__builtins__": {}}, dict(turns)))


# ---------------------------------------------------------------------- 1. where the kernels turn
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "block-1", "block", "block+1", "2*block+1"])
def test_record_counts_where_the_add_kernel_turns(engine, turns, tmp_path, size):
    n = sized(turns, size)
    lengths = [3000, 2000]
    records = spread(n, lengths, 100 + n)
    records[-1] = (0, 0, 1, lengths[1] - 50, [(M, 50)])               # (the last lane's record is counted, whatever chance gave)
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths)
    assert add_file(engine, tmp_path / "in.bam") == [n]
    want = check(collect(engine, lengths), records, lengths)
    assert want["counts"]["counted"] >= 1


@pytest.mark.parametrize("size", ["tile-1", "tile", "tile+1", "3*tile+5"])
def test_reference_sizes_where_the_tiles_turn(engine, turns, tmp_path, size):
    lengths = [sized(turns, size)]
    records = spread(600, lengths, 7) + [(0, 0, 0, 0, [(M, lengths[0])]), (0, 1, 0, lengths[0] - 1, [(M, 1)]), (0, 2, 0, 0, [(M, 1)])]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths)
    add_file(engine, tmp_path / "in.bam")
    want = check(collect(engine, lengths), records, lengths)
    assert want["per_contig"][0, 1] == lengths[0] and want["hist"][0] == 0


ROUND_SIZES = ["4*tile-1", "4*tile", "4*tile+1", "9*tile+3"]


def round_case(turns, size):
    lengths = [sized(turns, size)]
    return lengths, spread(900, lengths, 11) + [(0, 1, 0, lengths[0] - 1, [(M, 1)]), (0, 2, 0, 0, [(M, 1)])]


@pytest.fixture(scope="module")
def rounds_of_four(turns, tmp_path_factory):
    """A child process whose scan takes four tiles a round (MDX_TEST_DEPTH_ROUND is read where the accumulator is allocated):
    the four references, one after the other, what ``collect`` gives for each in an .npz."""
    d = tmp_path_factory.mktemp("rounds")
    for size in ROUND_SIZES:
        lengths, records = round_case(turns, size)
        write_records(d / (size.replace("*", "x") + ".bam"), records, names_of(lengths), lengths)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_depth_worker.py"), str(d)] +
                          ["%s:%d" % (size.replace("*", "x"), sized(turns, size)) for size in ROUND_SIZES],
                          cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_DEPTH_ROUND="4"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    return d


@pytest.mark.parametrize("size", ROUND_SIZES)
def test_reference_sizes_where_the_scan_turns(turns, rounds_of_four, size):
    lengths, records = round_case(turns, size)
    z = np.load(rounds_of_four / (size.replace("*", "x") + ".npz"))
    assert int(z["info"][2]) == 4 and int(z["info"][1]) == turns["tile"]
    got = dict(fetch=[z["fetch"]], per_contig=z["per_contig"], hist=z["hist"],
               counts=dict(zip(("counted", "outside", "intervals", "runs"), (int(x) for x in z["counts"]))),
               runs=(z["run_tid"], z["run_start"], z["run_end"], z["run_depth"]))
    want = check(got, records, lengths)
    # (depth beyond the first round's tiles: a carry that is lost shows there)
    assert want["depth"][0][4 * turns["tile"]:].any() or lengths[0] <= 4 * turns["tile"]


# ---------------------------------------------------------------------- 2. boundaries
def test_sequence_boundaries(engine, turns, tmp_path):
    """Five sequences, one of a single base and two empty ones in a row (names the FASTA lacks).  The first boundary lies exactly
    on a tile's edge, the next one base further — in the middle of a tile."""
    tile = turns["tile"]
    lengths = [tile, 1, 0, 0, 3000]
    names = names_of(lengths)
    full = reference(lengths)
    fasta.write_fasta(tmp_path / "ref.fa", Reference([names[t] for t in (0, 1, 4)], [full.seqs[t] for t in (0, 1, 4)]))
    ref = fasta.FastaOnDisk(tmp_path / "ref.fa", names, lengths, missing_ok=True)
    engine.set_reference(ref)
    assert ref.lengths == lengths
    engine.depth_begin()
    records = [
        (0, 0, 0, tile - 10, [(M, 10)]), (0, 1, 1, 0, [(M, 1)]),              # the last base of seq0, the first of seq1: -1 and +1 on one element
        (0, 2, 4, 0, [(M, 7)]),                                               # ... and seq1's only base and seq4's first, over the empty ones
        (0, 0, 4, 0, [(M, 3000)]),                                            # one read covers a whole sequence
        (0, 0, 0, 0, [(M, 5)]),                                               # begins at base 0
        (0, 1, 4, 2990, [(S, 3), (M, 10)]),                                   # ends at the length
        (0, 0, 2, 0, [(M, 1)]), (0, 0, 3, 0, [(M, 1)]),                       # on an empty sequence: outside
        (0, 0, 1, 0, [(M, 2)]), (0, 0, 1, 1, [(M, 1)]),                       # beyond the single base: outside
    ] + spread(300, lengths, 3)
    write_records(tmp_path / "in.bam", records, names, lengths)
    add_file(engine, tmp_path / "in.bam")
    got = collect(engine, lengths)
    want = check(got, records, lengths)
    assert want["counts"]["outside"] == 4 and got["per_contig"][2:4].tolist() == [[0, 0, 0, 0]] * 2
    assert got["fetch"][0][-1] >= 1 and got["fetch"][1][0] >= 1 and got["fetch"][4][0] >= 2
    # the runs on either side of a boundary stay two, whatever their depths
    tid, start, end, depth = got["runs"]
    assert ((tid == 1) & (start == 0) & (end == 1)).sum() == 1 and ((tid == 0) & (end == tile)).sum() == 1 and ((tid == 4) & (start == 0)).sum() == 1


# ---------------------------------------------------------------------- 3. contention
def test_one_record_twenty_thousand_times(engine, tmp_path):
    lengths = [2000, 1000]
    records = [(0, 1, 0, 500, [(M, 30), (D, 2), (M, 20)])] * 20_000
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths)
    assert len(add_file(engine, tmp_path / "in.bam")) == 1
    got = collect(engine, lengths)
    check(got, records, lengths)
    assert got["per_contig"][0].tolist() == [20_000, 50, 1_000_000, 20_000]
    assert got["hist"][1023] == 50 and got["hist"][0] == 2950 and got["hist"].sum() == 3000 and not got["hist"][1:1023].any()
    assert [a.tolist() for a in got["runs"]] == [[0, 0], [500, 532], [530, 552], [20_000, 20_000]]


def test_twenty_thousand_records_over_two_hundred_starts(engine, tmp_path):
    """Starts 3 apart under reads of 50: depths climb from 100 to 1 700, through bin 1022 into the last one."""
    lengths = [2000, 1000]
    records = [(0x10 * (m % 2), m % 3, 0, 100 + 3 * m, [(M, 50)]) for _ in range(100) for m in range(200)]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    begin(engine, lengths)
    add_file(engine, tmp_path / "in.bam")
    got = collect(engine, lengths)
    want = check(got, records, lengths)
    assert got["per_contig"][0, 3] == 1700 and got["hist"][1023] == (want["depth"][0] >= 1023).sum() > 300
    assert got["hist"][1000] == 3 * 2 and got["hist"][100] == 3 * 2 and got["hist"][1022] == 0


# ---------------------------------------------------------------------- 4. the rule on the device
def test_hand_written_records_on_the_device(engine, tmp_path):
    """The CPU test's records as a file.  Its header names one sequence more than the reference holds, so that a record can
    carry tid = n_contig; the neighbouring sequence is untouched by the records that end at, or reach beyond, the first one's end."""
    records = [r for r, _, _ in HAND]
    write_records(tmp_path / "in.bam", records, names_of(HAND_LENGTHS + [50]), HAND_LENGTHS + [50])
    begin(engine, HAND_LENGTHS)
    add_file(engine, tmp_path / "in.bam")
    got = collect(engine, HAND_LENGTHS)
    want = check(got, records, HAND_LENGTHS, HAND_LIBRARIES)
    assert got["counts"]["counted"] == [k for _, k, _ in HAND].count(PR.COUNTED) and got["counts"]["outside"] == [k for _, k, _ in HAND].count(PR.OUTSIDE)
    assert got["counts"]["intervals"] == sum(len(iv) for _, _, iv in HAND)
    # seq1 holds its own three records and nothing of seq0's
    only = PR.brute([r for r in records if r[2] == 1], HAND_LIBRARIES, HAND_LENGTHS)
    assert (got["fetch"][1].astype(np.int64) == only["depth"][1]).all() and (want["depth"][1] == only["depth"][1]).all()


# ---------------------------------------------------------------------- 5. slabs, order, state
@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    lengths = [30_000, 1, 12_000]
    records = spread(20_000, lengths, 41)
    d = tmp_path_factory.mktemp("depth_clustered")
    write_records(d / "in.bam", records, names_of(lengths), lengths)
    write_records(d / "reversed.bam", records[::-1], names_of(lengths), lengths)
    return dict(dir=d, records=records, lengths=lengths)


def test_one_slab_and_many_and_the_reversed_file(engine, clustered):
    lengths, records = clustered["lengths"], clustered["records"]
    begin(engine, lengths)
    assert len(add_file(engine, clustered["dir"] / "in.bam")) == 1
    one = collect(engine, lengths)
    again = collect(engine, lengths)                   # (a finish leaves the accumulator as it is)
    engine.depth_begin()                               # (a second begin zeroes it)
    assert len(add_file(engine, clustered["dir"] / "in.bam", 1 << 16)) >= 8
    many = collect(engine, lengths)
    engine.reset()
    add_file(engine, clustered["dir"] / "reversed.bam", 1 << 16)
    rev = collect(engine, lengths)
    check(one, records, lengths)
    for other in (again, many, rev):
        assert all((a == b).all() for a, b in zip(one["fetch"], other["fetch"])) and (one["per_contig"] == other["per_contig"]).all()
        assert (one["hist"] == other["hist"]).all() and one["counts"] == other["counts"]
        assert all((a == b).all() and len(a) == len(b) for a, b in zip(one["runs"], other["runs"]))


def test_a_finish_between_two_adds_and_reset(engine, clustered, tmp_path):
    lengths, records = clustered["lengths"], clustered["records"]
    write_records(tmp_path / "a.bam", records[:700], names_of(lengths), lengths)
    write_records(tmp_path / "b.bam", records[700:1500], names_of(lengths), lengths)
    begin(engine, lengths)
    add_file(engine, tmp_path / "a.bam")
    check(collect(engine, lengths), records[:700], lengths)
    add_file(engine, tmp_path / "b.bam")
    check(collect(engine, lengths), records[:1500], lengths)
    engine.reset()
    zero = collect(engine, lengths)
    check(zero, [], lengths)
    assert zero["counts"] == dict(counted=0, outside=0, intervals=0, runs=0) and zero["hist"][0] == sum(lengths) and len(zero["runs"][0]) == 0
    add_file(engine, tmp_path / "b.bam")
    check(collect(engine, lengths), records[700:1500], lengths)


def test_call_order(clustered):
    from mapdamage_amd.engine import DamageEngine, MdxError
    lengths = clustered["lengths"]
    with DamageEngine(LIBS3) as other:
        with pytest.raises(MdxError) as error:
            other.depth_begin()                        # no reference yet
        assert error.value.code == ERR_STATE
        other.set_reference(reference(lengths))
        with sam.GpuBamStream(other, str(clustered["dir"] / "in.bam"), readgroups=[(rg, i) for i, rg in enumerate(RG3)]) as stream:
            with pytest.raises(MdxError) as error:
                other.depth_add(stream.next_view())
        assert error.value.code == ERR_STATE and "mdx_depth_begin" in str(error.value)
        for call in (other.depth_finish, other.depth_runs, other.depth_info, lambda: other.depth_fetch(0, 0, 1)):
            with pytest.raises(MdxError) as error:
                call()
            assert error.value.code == ERR_STATE
        other.depth_begin()
        # a new reference releases the accumulator that was laid out by the old one
        other.set_reference(reference([500]))
        with pytest.raises(MdxError) as error:
            other.depth_finish()
        assert error.value.code == ERR_STATE


# ---------------------------------------------------------------------- 6. the final flags
def test_the_flags_as_they_stand(engine, clustered):
    """0x200 on chosen records in front of the add, as the draws of -n 0.5 leave them, and ``dedup_mark`` in front of it: the
    depth is the brute force over the records that survive both."""
    lengths = clustered["lengths"]
    rng = np.random.default_rng(9)
    # (4 000 records and 2 000 copies of some of them, anywhere in the file)
    records = [clustered["records"][j] for j in rng.permutation(np.concatenate([np.arange(4000), rng.choice(4000, 2000)]))]
    drop = np.zeros(len(records), bool)
    drop[rng.choice(6000, 1500, replace=False)] = True

    def before(stream, view, first):
        f = stream.view_flags(view)
        f[drop[first:first + len(f)]] |= 0x200
        stream.set_view_flags(view, f)
        engine.dedup_mark(view)

    path = clustered["dir"] / "first.bam"
    write_records(path, records, names_of(lengths), lengths)
    begin(engine, lengths)
    engine.dedup_begin()
    assert len(add_file(engine, path, 1 << 16, before=before)) >= 3
    dropped = [(f | (0x200 if gone else 0), lib, t, p, c) for (f, lib, t, p, c), gone in zip(records, drop)]
    dup = DR.brute(dropped, 3)[0]
    assert 200 < dup.sum() < 4000
    survivors = [(f | (0x400 if d else 0), lib, t, p, c) for (f, lib, t, p, c), d in zip(dropped, dup)]
    want = check(collect(engine, lengths), survivors, lengths)
    assert want["counts"]["counted"] < PR.brute(records, 3, lengths)["counts"]["counted"] - 1500


# ---------------------------------------------------------------------- 7. the command line
def expected_files(out, names, lengths, records, n_libraries, bedgraph=None):
    want = PR.brute(records, n_libraries, lengths)
    assert (out / "coverage.tsv").read_text() == PR.coverage_text(names, lengths, want["per_contig"])
    assert (out / "depth_histogram.tsv").read_text() == PR.histogram_text(want["hist"])
    hist = [line.split("\t") for line in (out / "depth_histogram.tsv").read_text().splitlines()[1:]]
    assert sum(int(n) for _, n in hist) == sum(lengths)
    star = (out / "coverage.tsv").read_text().splitlines()[-1].split("\t")
    assert star[0] == "*" and int(star[1]) == sum(lengths)
    if bedgraph is not None:
        text = open(bedgraph).read()
        assert text == PR.bedgraph_text(names, want["runs"]) and text
        rows = [line.split("\t") for line in text.splitlines()]
        assert sum((int(e) - int(s)) * int(d) for _, s, e, d in rows) == int(star[5])
        assert os.listdir(os.path.dirname(bedgraph)) == [os.path.basename(bedgraph)]         # (no temporary file left)
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    total = want["per_contig"].sum(axis=0)
    assert "Depth: %d records, %d aligned bases; %d of %d reference bases covered" % (want["counts"]["counted"], total[2], total[1], sum(lengths)) in log
    assert "%d records outside their sequence" % want["counts"]["outside"] in log
    return want


def test_command_line(dup_data, tmp_path):
    ref, records = dup_data["ref"], dup_data["records"]
    names, lengths = list(ref.names), [int(x) for x in ref.lengths]
    with_option = run(dup_data, tmp_path / "with", "in.bam", "--depth", "--by-reference")
    without = run(dup_data, tmp_path / "without", "in.bam", "--by-reference")
    want = expected_files(with_option, names, lengths, records, 3)
    assert want["counts"]["counted"] > 1000 and (want["per_contig"][:, 0] > 0).all()
    # nothing else differs: the three usual files and groups.tsv byte for byte, and without the option neither file nor line
    assert tables(with_option) == tables(without)
    assert (with_option / "by_reference" / "groups.tsv").read_bytes() == (without / "by_reference" / "groups.tsv").read_bytes()
    assert not (without / "coverage.tsv").exists() and not (without / "depth_histogram.tsv").exists()
    assert "Depth:" not in (without / "Runtime_log.txt").read_text()


def test_command_line_behind_the_duplicates(dup_data, tmp_path):
    ref, records = dup_data["ref"], dup_data["records"]
    out = run(dup_data, tmp_path / "out", "in.bam", "--remove-duplicates", "--depth")
    dup = dup_data["both"][0]
    survivors = [(f | (0x400 if d else 0), lib, t, p, c) for (f, lib, t, p, c), d in zip(records, dup)]
    want = expected_files(out, list(ref.names), [int(x) for x in ref.lengths], survivors, 3)
    assert want["counts"]["counted"] < PR.brute(records, 3, ref.lengths)["counts"]["counted"] - 200


@pytest.mark.parametrize("route", ["file", "pipe"])
def test_command_line_with_a_filter_and_the_bedgraph(dup_data, tmp_path, route):
    ref, records = dup_data["ref"], dup_data["records"]
    (tmp_path / "bg").mkdir()
    bedgraph = tmp_path / "bg" / "x.bg"
    out = run(dup_data, tmp_path / "out", "in.bam", "--min-mapq", "25", "--depth", "--depth-bedgraph", bedgraph, route=route)
    seen = [(f | (0x200 if q < 25 else 0), lib, t, p, c) for (f, lib, t, p, c), q in zip(records, _mapq(dup_data))]
    expected_files(out, list(ref.names), [int(x) for x in ref.lengths], seen, 3, bedgraph=str(bedgraph))


def test_command_line_against_the_written_file(dup_data, tmp_path):
    """With --write-kept the written file holds the counted records: read back and brute-forced, it gives the run's own files."""
    ref = dup_data["ref"]
    kept = tmp_path / "kept.bam"
    out = run(dup_data, tmp_path / "out", "in.bam", "--remove-duplicates", "--min-mapq", "25", "--depth", "--write-kept", kept)
    written = []
    for r in read_bam_file(kept)[1]:
        tid, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", r, 4)
        words = struct.unpack_from("<%dI" % n_cigar, r, 36 + l_name)
        written.append((flag, 0, tid, pos, [(w & 15, w >> 4) for w in words]))
    assert len(written) > 500
    want = expected_files(out, list(ref.names), [int(x) for x in ref.lengths], written, 1)
    assert want["counts"]["counted"] == len(written) and want["counts"]["outside"] == 0


def test_sam_text_is_refused(dup_data, tmp_path):
    from tests.test_gpu_write_kept import RGS
    b, ref = dup_data["batch"].slice(0, 200), dup_data["ref"]
    sam.write_sam(str(tmp_path / "in.sam"), b, ref.names, ref.lengths, RGS, [RGS[int(i)]["ID"] for i in b.lib])
    out = run(dup_data, tmp_path / "sam", tmp_path / "in.sam", "--depth", rc=1)
    assert "--depth needs BAM input" in (out / "Runtime_log.txt").read_text()
    assert not any((out / f).exists() for f in FILES + ("coverage.tsv", "depth_histogram.tsv"))


def test_a_slab_the_device_path_gives_up_on_ends_the_run(dup_data, tmp_path, monkeypatch):
    from mapdamage_amd.main import main
    monkeypatch.setenv("MDX_GBAM_FAIL_AT", "0")             # (its first slab)
    out = tmp_path / "out"
    assert main(["-i", str(dup_data["dir"] / "in.bam"), "-r", str(dup_data["dir"] / "ref.fa"), "-d", str(out), "--no-stats", "--depth",
                 "--depth-bedgraph", str(tmp_path / "x.bg")]) == 1
    monkeypatch.delenv("MDX_GBAM_FAIL_AT")
    log = (out / "Runtime_log.txt").read_text()
    assert "GPU decode path gave up" in log
    assert "--depth is gathered on the device decode path" in log.split("GPU decode path gave up")[1]
    assert not any((out / f).exists() for f in FILES + ("coverage.tsv", "depth_histogram.tsv")) and not (tmp_path / "x.bg").exists()
