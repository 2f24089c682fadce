"""--write-index on the GPU (include/mdx.h ``mdx_gbam_kept_index`` / ``mdx_gbam_kept_index_linear``; csrc/mdx_kept_index.h;
mapdamage_amd/bai.py): the BAI index of the file --write-kept writes, from the offsets and columns the run has on the device.

In every case the index must be byte for byte what the yardstick (tests/bai_util.py: from the SAM specification, sharing nothing
with the product) derives from the WRITTEN file alone, and a reader that goes through the index must find what a scan of the file
finds.  The files are made by the builders of tests/test_write_index.py, in coordinate order.

The kernels' constants (csrc/mdx_gbam.hip): KEPT_TILE records per block, KEPT_SCAN_ROUND tiles per round of the one block that
scans the tile sums — 65 536 written records pass one round."""

import dataclasses
import struct

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from mapdamage_amd.bai import BaiAssembler, member_sizes
from tests import bai_util as Y
from tests import regions_util as R
from tests.test_gpu_record_filters import ARGS
from tests.test_gpu_strata import MIXED, genome5
from tests.test_gpu_write_kept import DEVICE, EOF_MARKER, FILES, RGS, lib_stream, patterns, run, strata_engine, tables
from tests.test_write_index import MEMBER, border_slabs, record, write_sorted_input

pytestmark = pytest.mark.gpu

KEPT_TILE, KEPT_SCAN_ROUND = 256, 256
TOP = 1 << 29
DROP_BITS = (0x4, 0x100, 0x200, 0x400, 0x800)


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("s", "l")]) as eng:
        yield eng


def open_stream(eng, path, chunk_bytes=256 << 20):
    return sam.GpuBamStream(eng, str(path), readgroups=[("rgA", 0)], lib_default=0, chunk_bytes=chunk_bytes)


def write_and_index(eng, stream, out_path, before_write=None, **write_kw):
    """What main.py's _KeptOutput does, at the library level: every slab's kept records behind the header, the index entries of
    each slab right behind its write.  Returns (index bytes, slabs that wrote records, all slabs)."""
    header = bytes(eng.bgzf_deflate(sam.bam_header_bytes(stream.header)))
    asm = BaiAssembler(stream.header.lengths)
    pieces, base, file_at, prev, n_slabs, n_views = [header], 0, len(header), (-1, -1), 0, 0
    while True:
        view = stream.next_view()
        if view is None:
            break
        n_views += 1
        if before_write is not None:
            before_write(view)
        members, n, raw = stream.write_kept(view, **write_kw)
        runs, new_prev = stream.kept_index(base, prev, n)
        if n:
            assert new_prev != (-1, -1) and 1 <= len(runs) <= n and int(runs["last"][-1]) == n and int(runs["first"][0]) == 0
            asm.add_slab(base, file_at, member_sizes(members), raw, runs)
            n_slabs += 1
        else:
            assert len(runs) == 0 and new_prev == prev
        prev = new_prev
        base += raw
        file_at += len(members)
        pieces.append(bytes(members))
    index = asm.finish(stream.kept_index_linear())
    with open(out_path, "wb") as out:
        out.write(b"".join(pieces) + EOF_MARKER)
    return index, n_slabs, n_views


def index_of(eng, path, out_path, chunk_bytes=256 << 20):
    with open_stream(eng, path, chunk_bytes) as stream:
        return write_and_index(eng, stream, out_path)


def check(eng, path, out_path, n_kept, chunk_bytes=256 << 20, regions=()):
    """The product's index of the file it writes against the yardstick's; returns (Bam, parsed index, slabs with records)."""
    got, n_slabs, _ = index_of(eng, path, out_path, chunk_bytes)
    bam = Y.Bam(out_path)
    assert len(bam.records) == n_kept
    want = Y.build_index(bam)
    assert got == want, first_difference(got, want)
    parsed = Y.parse_index(got)
    for tid, beg, end in regions:
        assert Y.query(bam, parsed, tid, beg, end) == Y.brute(bam, tid, beg, end), (tid, beg, end)
    return bam, parsed, n_slabs


def first_difference(got, want):
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "lengths %d and %d, first difference at byte %d: %s against %s" % (len(got), len(want), at, got[at:at + 24].hex(), want[at:at + 24].hex())


def with_flags(records, keep):
    """A dropped record gets one of the five bits of 0xF04, in turn."""
    out, k = [], 0
    for r, stay in zip(records, keep):
        if not stay:
            r = r[:18] + struct.pack("<H", struct.unpack_from("<H", r, 18)[0] | DROP_BITS[k % 5]) + r[20:]
            k += 1
        out.append(r)
    return out


# ---------------------------------------------------------------------- 1. runs, windows, bins
def border_records(tids):
    """On each of ``tids``: records that end on, start on, straddle and end one behind a border of every level of the binning
    scheme, records without a reference base on both sides of it, a skip across most of the sequence — in coordinate order."""
    found = []
    for shift in (14, 17, 20, 23, 26):
        for k in (1, 3, (TOP >> shift) - 1):
            border = k << shift
            found += [(border - 100, [(100, "M")]), (border - 99, [(60, "M"), (2, "I"), (40, "=")]), (border - 50, [(30, "M"), (40, "D"), (30, "X")]),
                      (border, [(100, "M")]), (border - 1, []), (border, [(7, "S")]), (border - 1, [(1, "M"), (9, "S")]), (border - 1, [(2, "M")])]
    # (an operation's length has 28 bits: the skip takes two)
    found += [(1000, [(10, "M"), ((1 << 28) - 1, "N"), (TOP - 5000 - (1 << 28) + 1, "N"), (10, "M")]), (0, [(1, "M")]), (TOP - 1, []), (TOP - 16_384, [(16_384, "M")])]
    found.sort(key=lambda f: f[0])
    return [record(tid, pos, cigar, b"t%d_%d" % (tid, i), size=60 + 4 * len(cigar) + (i * 37) % 300)
            for tid in tids for i, (pos, cigar) in enumerate(found)]


BORDER_REGIONS = [(0, 0, TOP), (0, 16_383, 16_385), (0, 1 << 26, (1 << 26) + 1), (0, (1 << 26) - 1, 1 << 26), (0, 5000, 6000), (0, TOP - 1, TOP),
                  (0, 3 << 20, (3 << 20) + 1), (1, 0, TOP), (1, 3 << 23, (3 << 23) + 100), (2, 0, 1), (2, 0, TOP), (2, (1 << 14) - 1, 1 << 14),
                  (0, 2 << 20, (2 << 20) + 5), (1, 100, 200), (2, 200_000_000, 300_000_000), (0, 16_384, 16_385), (2, 131_071, 131_073)]


@pytest.mark.parametrize("tids", [(0, 2), (1, 2), (0, 1), (0, 1, 2), (1,)])
def test_borders_of_every_level(engine, tmp_path, tids):
    refs = [("chr1", TOP), ("chr2", TOP), ("chr3", TOP)]
    records = border_records(tids)
    write_sorted_input(tmp_path / "in.bam", refs, records, block_bytes=3001)
    bam, parsed, _ = check(engine, tmp_path / "in.bam", tmp_path / "kept.bam", len(records), regions=BORDER_REGIONS)
    assert [r["bytes"] for r in bam.records] == records
    for tid in range(3):
        bins, linear = parsed[tid]
        if tid not in tids:
            assert bins == {} and linear == []
            continue
        assert len(linear) == TOP >> 14 and bins[37450][1] == (len(records) // len(tids), 0)
        levels = {sum(b >= o for o in (1, 9, 73, 585, 4681)) for b in bins if b != 37450}
        assert levels == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("n", [1, KEPT_TILE - 1, KEPT_TILE, KEPT_TILE + 1])
def test_keep_patterns(engine, tmp_path, n):
    """Every pattern of kept and dropped records around one tile; the dropped ones out of order and out of every sequence, which
    nobody looks at."""
    refs = [("chr1", 400_000), ("chr2", 1000), ("chr3", 50_000)]
    rng = np.random.default_rng(n)
    tid = np.sort(rng.choice([0, 2], n))
    pos = np.concatenate([np.sort(rng.integers(0, refs[t][1] - 700, int((tid == t).sum()))) for t in (0, 2)])
    plain = [record(int(t), int(p), [(int(rng.integers(1, 600)), "M")], b"p%d" % i, size=70 + i % 90) for i, (t, p) in enumerate(zip(tid, pos))]
    stray = [record(0, 399_990, [(500, "M")], b"stray0", size=80), record(-1, -1, [], b"stray1"), record(2, 10, [(100_000, "N")], b"stray2", size=90)]
    for name, keep in patterns(n).items():
        records = [stray[i % 3] if not k else r for i, (r, k) in enumerate(zip(plain, keep))]
        records = with_flags(records, keep)
        path = tmp_path / ("%s.bam" % name.replace(" ", "_"))
        write_sorted_input(path, refs, records, block_bytes=3001)
        bam, parsed, _ = check(engine, path, tmp_path / "kept.bam", int(keep.sum()),
                               regions=[(0, 0, 400_000), (0, 16_000, 17_000), (1, 0, 1000), (2, 0, 50_000), (2, 49_000, 50_000), (0, 200_000, 200_001)])
        assert [r["bytes"] for r in bam.records] == [r for r, k in zip(records, keep) if k]


def test_more_records_than_a_scan_round(engine, tmp_path):
    """70 000 minimal records in one slab, nearly all of them written: 266 tiles of written records, two rounds of the one block
    that scans the tile sums — of the kept kernels' and of the index kernels'."""
    n = 70_000
    refs = [("chr1", 1 << 22), ("chr2", 1 << 20)]
    rng = np.random.default_rng(70)
    keep = rng.random(n) < 0.97
    tid = (np.arange(n) >= 50_000).astype(int)
    pos = np.concatenate([np.sort(rng.integers(0, (1 << 22) - 200, 50_000)), np.sort(rng.integers(0, (1 << 20) - 200, 20_000))])
    span = rng.integers(1, 150, n)
    records = with_flags([record(int(t), int(p), [(int(s), "M")], b"%d" % (i % 10)) for i, (t, p, s) in enumerate(zip(tid, pos, span))], keep)
    assert keep.sum() > KEPT_TILE * KEPT_SCAN_ROUND and max(len(r) for r in records) <= 42
    write_sorted_input(tmp_path / "in.bam", refs, records, block_bytes=60_000, level=1)
    regions = [(0, 0, 1 << 22), (1, 0, 1 << 20), (0, 1 << 21, (1 << 21) + 100), (1, 500_000, 500_010), (0, (1 << 22) - 100, 1 << 22)]
    bam, parsed, n_slabs = check(engine, tmp_path / "in.bam", tmp_path / "kept.bam", int(keep.sum()), regions=regions)
    assert n_slabs == 1 and len(parsed[0][1]) == 256 and len(parsed[1][1]) == 64
    assert sum(len(c) for b, c in parsed[0][0].items() if b != 37450) > 256          # more runs than windows: records across their borders


# ---------------------------------------------------------------------- 2. member borders
@pytest.mark.parametrize("ends_on_a_border", [True, False])
def test_member_borders(engine, tmp_path, ends_on_a_border):
    """One slab whose stream has a record that ends exactly at 0xFF00, one that straddles 2 * 0xFF00, and whose last record ends
    on a member border (three full members) or inside a member."""
    refs, slabs = border_slabs()
    records = slabs[0] if ends_on_a_border else slabs[0] + slabs[2]
    assert (sum(len(r) for r in records) % MEMBER == 0) == ends_on_a_border
    write_sorted_input(tmp_path / "in.bam", refs, records, block_bytes=30_011)
    bam, parsed, n_slabs = check(engine, tmp_path / "in.bam", tmp_path / "kept.bam", len(records),
                                 regions=[(0, 0, TOP), (0, 100_000, 100_001), (0, 170_000, 171_000), (0, TOP - 1, TOP), (1, 0, 5000), (2, 0, 1),
                                          (2, 117_005, 117_006)])
    assert n_slabs == 1
    data_members = [m for m in bam.members[1:-1]]
    assert [m[3] for m in data_members[:3]] == [MEMBER] * 3 and len(data_members) == (3 if ends_on_a_border else 4)
    ends = [c[1] for bins, _ in parsed for b, cs in bins.items() for c in cs]
    assert max(ends) == bam.members[-1][0] << 16                  # the last record ends at the marker
    # the record that ends at 0xFF00 of the stream ends at the second data member's first byte
    stops = {bam.virtual(r["stop"]) for r in bam.records}
    assert data_members[1][0] << 16 in stops and (data_members[2][0] << 16) not in stops


# ---------------------------------------------------------------------- 3. several slabs
def positions_of(bam, parsed):
    """The parsed index with every virtual offset turned into a place in the inflated data: what does not depend on how the
    file is cut into members."""
    at = {m[0]: m[2] for m in bam.members}
    place = lambda v: at[v >> 16] + (v & 0xFFFF)       # noqa: E731
    return [({b: [(place(c[0]), place(c[1])) if b != 37450 or k == 0 else c for k, c in enumerate(cs)] for b, cs in bins.items()},
             [place(v) for v in linear]) for bins, linear in parsed]


def test_several_slabs(engine, tmp_path):
    refs = [("chr1", 3_000_000), ("chr2", 100), ("chr3", 600_000)]
    rng = np.random.default_rng(31)
    n = 4000
    tid = np.where(np.arange(n) < 3000, 0, 2)
    pos = np.concatenate([np.sort(rng.integers(0, 2_990_000, 3000)), np.sort(rng.integers(0, 590_000, 1000))])
    records = [record(int(t), int(p), [(int(rng.integers(1, 5000)), "M")], b"s%d" % i, size=100 + int(rng.integers(0, 300)))
               for i, (t, p) in enumerate(zip(tid, pos))]
    keep = rng.random(n) < 0.8
    keep[1000:1700] = False                 # slabs without a written record between slabs with some
    records = with_flags(records, keep)
    write_sorted_input(tmp_path / "in.bam", refs, records, block_bytes=5000, level=0)
    regions = [(0, 0, 3_000_000), (0, 1_500_000, 1_500_100), (1, 0, 100), (2, 0, 600_000), (2, 300_000, 310_000), (0, 16_384, 32_768)]
    one, parsed_one, n_one = check(engine, tmp_path / "in.bam", tmp_path / "one.bam", int(keep.sum()), regions=regions)
    many, parsed_many, n_many = check(engine, tmp_path / "in.bam", tmp_path / "many.bam", int(keep.sum()), chunk_bytes=65536, regions=regions)
    assert n_one == 1 and n_many >= 6
    assert one.stream == many.stream and len(many.members) > len(one.members)
    # the same chunks and the same windows, wherever the slabs ended: a run that crosses a slab border is one chunk, and a
    # window first touched in an earlier slab keeps that record's offset
    assert positions_of(one, parsed_one) == positions_of(many, parsed_many)
    # ... and runs did cross slab borders: the slabs' first members lie inside chunks
    slab_firsts = []
    for m, before in zip(many.members[1:-1], many.members[:-2]):
        if before[3] != MEMBER and before[0] != 0:
            slab_firsts.append(m[0])
    assert len(slab_firsts) >= 5
    chunks = [c for bins, _ in parsed_many for b, cs in bins.items() if b != 37450 for c in cs]
    assert sum(1 for f in slab_firsts if any(c[0] >> 16 < f <= c[1] >> 16 and c[1] > f << 16 for c in chunks)) >= 3


# ---------------------------------------------------------------------- 4. selection and tags
@pytest.fixture(scope="module")
def sorted_data(tmp_path_factory):
    """A few thousand records over genome5() in three libraries in coordinate order, with qualities, MAPQ and extra flag bits."""
    d = tmp_path_factory.mktemp("write_index")
    ref = genome5()
    rng = np.random.default_rng(2027)
    b = synth.make_reads(ref, 3000, 94, nlib=3, with_qual=True, sort=True, **dict(MIXED, len_range=(30, 150)))
    assert (np.diff(b.tid.astype(np.int64) * (1 << 32) + b.pos) >= 0).all()
    nb = b.seq.shape[0]
    b.qual = np.where(rng.random(nb) < 0.05, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    flag16 = b.flag.astype(np.int64)
    for bit in (0x1, 0x400, 0x800):
        flag16 |= np.where(rng.random(b.n) < 0.1, bit, 0)
    mapq = rng.choice((0, 1, 24, 25, 29, 30, 37, 60, 255), b.n)
    b = dataclasses.replace(b, flag=flag16.astype(np.uint16))
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    fasta.write_fasta(d / "ref.fa", ref)
    (d / "panels.bed").write_text(R.bed_text(R.grid_regions(), ref.names, R.GRID_GROUPS))
    # the same records in another order: what the refusals need
    u = synth.make_reads(ref, 600, 95, nlib=3, with_qual=True, **dict(MIXED, len_range=(30, 150)))
    sam.write_bam(str(d / "unsorted.bam"), u, ref.names, ref.lengths, RGS, [RGS[int(i)]["ID"] for i in u.lib])
    return dict(dir=d, ref=ref, batch=b, unsorted=u)


CLI_CASES = {
    "pmd tags": ["--by-pmd-score", "--write-groups", "1", "--tag-group", "XG", "--tag-pmd-score", "DS"],
    "regions": ["--regions", "panels.bed", "--write-groups", "0"],
    "filters": ARGS["all"] + ["-n", "0.5", "--downsample-seed", "7"],
    "only regions": ["--regions", "panels.bed", "--only-regions", "-Q", "20", "--chunk-mb", "64"],
}


@pytest.mark.parametrize("slabs", [False, True])
@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_command_line(sorted_data, tmp_path, monkeypatch, case, slabs):
    if slabs:
        monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    opts = [str(sorted_data["dir"] / a) if a.endswith(".bed") else a for a in CLI_CASES[case]]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = run(sorted_data, tmp_path / "out_plain", "in.bam", *opts, "--write-kept", tmp_path / "a" / "kept.bam")
    out = run(sorted_data, tmp_path / "out", "in.bam", *opts, "--write-kept", tmp_path / "b" / "kept.bam", "--write-index")
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["kept.bam"]
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["kept.bam", "kept.bam.bai"]           # no temporary file is left
    kept = tmp_path / "b" / "kept.bam"
    assert kept.read_bytes() == (tmp_path / "a" / "kept.bam").read_bytes()
    assert tables(out) == tables(plain)
    assert (out / "write_kept.tsv").read_text().replace(str(tmp_path / "b"), "") == (plain / "write_kept.tsv").read_text().replace(str(tmp_path / "a"), "")
    bam = Y.Bam(kept)
    assert 100 < len(bam.records) < 3000
    got = (tmp_path / "b" / "kept.bam.bai").read_bytes()
    want = Y.build_index(bam)
    assert got == want, first_difference(got, want)
    parsed = Y.parse_index(got)
    n_refs = sum(1 for bins, _ in parsed if bins)
    n_chunks = sum(len(c) for bins, _ in parsed for b, c in bins.items() if b != 37450)
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    assert "Wrote index %s.bai (%d references with records, %d chunks)" % (kept, n_refs, n_chunks) in log
    assert "Wrote index" not in (plain / "Runtime_log.txt").read_text()
    rng = np.random.default_rng(len(case))
    lengths = sorted_data["ref"].lengths
    for _ in range(30):
        tid = int(rng.integers(0, len(lengths)))
        beg = int(rng.integers(0, lengths[tid]))
        end = min(int(lengths[tid]), beg + int(rng.choice([1, 30, 2000])))
        assert Y.query(bam, parsed, tid, beg, end) == Y.brute(bam, tid, beg, end), (tid, beg, end)


def test_tags_at_the_library_level(sorted_data, tmp_path):
    """A selection and both tags: the index is that of the TAGGED records' file (twelve bytes more per record)."""
    eng, n_groups = strata_engine("pmd", sorted_data["ref"])
    with eng:
        eng.keep_pmd_scores(True)
        with lib_stream(eng, sorted_data["dir"] / "in.bam", "pmd") as stream:
            index, n_slabs, n_views = write_and_index(eng, stream, tmp_path / "kept.bam", before_write=eng.tabulate_view, groups=(1, 2),
                                                      n_groups=n_groups, group_tag="XG", score_tag="DS")
            eng.sync()
    assert n_views >= 3 and n_slabs >= 3            # (sorted records compress well: three slabs of 64 KiB, each with written records)
    bam = Y.Bam(tmp_path / "kept.bam")
    assert len(bam.records) > 100 and all(r["bytes"][-12:-10] == b"XG" and r["bytes"][-7:-4] == b"DSf" for r in bam.records)
    want = Y.build_index(bam)
    assert index == want, first_difference(index, want)


# ---------------------------------------------------------------------- 5. refusals
REFS = [("chr1", 100_000), ("chr2", 50_000)]


def slab_counts(eng, path, chunk_bytes):
    counts = []
    with open_stream(eng, path, chunk_bytes) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                return counts
            counts.append(int(view.n_reads))


def refusal_of(eng, path, chunk_bytes=256 << 20):
    """(KeptIndexError, views handed out before it)"""
    with open_stream(eng, path, chunk_bytes) as stream:
        with pytest.raises(sam.KeptIndexError) as err:
            write_and_index(eng, stream, str(path) + ".out")
    assert err.value.code == -6
    return err.value


def test_refusals(engine, tmp_path):
    rng = np.random.default_rng(8)
    n = 1500
    pos = np.sort(rng.integers(0, 99_000, n))
    plain = [record(0, int(p), [(50, "M")], b"n%d" % i, size=150 + i % 100) for i, p in enumerate(pos)]
    write_sorted_input(tmp_path / "ok.bam", REFS, plain, block_bytes=5000, level=0)
    counts = slab_counts(engine, tmp_path / "ok.bam", 65536)
    assert len(counts) >= 3 and sum(counts) == n
    check(engine, tmp_path / "ok.bam", tmp_path / "ok.kept.bam", n, chunk_bytes=65536)

    def moved(i, new_pos, flag=0, cigar=((50, "M"),)):
        return record(0, new_pos, list(cigar), b"n%d" % i, flag=flag, size=len(plain[i]))

    # two written records out of order inside a slab (the blocks are stored: the slabs' borders do not move with the bytes)
    k = counts[0] + 5
    assert pos[k] > 10
    records = plain[:k] + [moved(k, int(pos[k - 1]) - 1)] + plain[k + 1:]
    write_sorted_input(tmp_path / "inside.bam", REFS, records, block_bytes=5000, level=0)
    assert slab_counts(engine, tmp_path / "inside.bam", 65536) == counts
    err = refusal_of(engine, tmp_path / "inside.bam", 65536)
    assert (err.index, err.name, err.reason) == (5, "n%d" % k, sam.KeptIndexError.UNSORTED) and "coordinate order" in str(err)
    err = refusal_of(engine, tmp_path / "inside.bam")                 # ... and in one slab
    assert (err.index, err.name, err.reason) == (k, "n%d" % k, sam.KeptIndexError.UNSORTED)
    # ... across a slab border: the slab's first written record against the last one of the slab in front
    k = counts[0] + counts[1]
    records = plain[:k] + [moved(k, int(pos[k - 1]) - 1)] + plain[k + 1:]
    write_sorted_input(tmp_path / "across.bam", REFS, records, block_bytes=5000, level=0)
    assert slab_counts(engine, tmp_path / "across.bam", 65536) == counts
    err = refusal_of(engine, tmp_path / "across.bam", 65536)
    assert (err.index, err.name, err.reason) == (0, "n%d" % k, sam.KeptIndexError.UNSORTED)
    # ... with dropped records between the two
    records = plain[:k - 3] + with_flags(plain[k - 3:k], [False] * 3) + with_flags(plain[k:k + 2], [False] * 2) + [moved(k + 2, int(pos[k - 4]) - 1)] + plain[k + 3:]
    write_sorted_input(tmp_path / "across2.bam", REFS, records, block_bytes=5000, level=0)
    err = refusal_of(engine, tmp_path / "across2.bam", 65536)
    assert (err.index, err.name, err.reason) == (2, "n%d" % (k + 2), sam.KeptIndexError.UNSORTED)
    # a written record that ends behind its sequence; the lowest of two offenders is reported
    k = n - 2
    records = plain[:k] + [moved(k, 99_950), moved(k + 1, 99_970, cigar=((30, "M"),))]
    write_sorted_input(tmp_path / "end.bam", REFS, records, block_bytes=5000, level=0)
    check(engine, tmp_path / "end.bam", tmp_path / "end.kept.bam", n)                     # (both end exactly at LN: fine)
    records = plain[:k] + [moved(k, 99_951), moved(k + 1, 99_970, cigar=((31, "M"),))]
    write_sorted_input(tmp_path / "end.bam", REFS, records, block_bytes=5000, level=0)
    err = refusal_of(engine, tmp_path / "end.bam")
    assert (err.index, err.name, err.reason) == (k, "n%d" % k, sam.KeptIndexError.UNPLACEABLE) and "reference sequence" in str(err)
    # an out-of-order record that is dropped is no error, nor is one outside every sequence
    k = counts[0] + 7
    records = plain[:k] + [moved(k, 3, flag=0x400), moved(k + 1, 99_990, flag=0x200, cigar=((5000, "M"),))] + plain[k + 2:]
    write_sorted_input(tmp_path / "dropped.bam", REFS, records, block_bytes=5000, level=0)
    check(engine, tmp_path / "dropped.bam", tmp_path / "dropped.kept.bam", n - 2, chunk_bytes=65536)


def test_state_and_empty_results(engine, tmp_path):
    from mapdamage_amd.engine import MdxError
    plain = [record(0, 10 * i, [(50, "M")], b"n%d" % i, size=200) for i in range(1200)]
    write_sorted_input(tmp_path / "in.bam", REFS, plain, block_bytes=5000, level=0)
    with open_stream(engine, tmp_path / "in.bam", 65536) as stream:
        assert (stream.kept_index_linear() == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and len(stream.kept_index_linear()) == 7 + 4
        view = stream.next_view()
        with pytest.raises(MdxError, match="write the view first") as err:          # nothing written yet
            stream.kept_index(0, (-1, -1), 10)
        assert err.value.code == -3
        members, n, raw = stream.write_kept(view)
        with pytest.raises(MdxError, match="runs") as err:                          # an array that is too small
            _small_array(stream, n)
        assert err.value.code == -1
        runs, prev = stream.kept_index(0, (-1, -1), n)
        assert len(runs) >= 1 and prev == (0, 10 * (n - 1)) and int(runs["uend"][-1]) == raw and int(runs["ustart"][0]) == 0
        view = stream.next_view()                                                    # the next view: the write was the last one's
        with pytest.raises(MdxError, match="write the view first") as err:
            stream.kept_index(raw, prev, n)
        assert err.value.code == -3
        stream.write_kept(view)
        assert len(stream.kept_index(raw, prev, int(view.n_reads))[0]) >= 1
    # nothing is written: a valid file, an index without bins
    write_sorted_input(tmp_path / "none.bam", REFS, with_flags(plain, [False] * len(plain)), block_bytes=5000, level=0)
    bam, parsed, n_slabs = check(engine, tmp_path / "none.bam", tmp_path / "none.kept.bam", 0, chunk_bytes=65536, regions=[(0, 0, 100_000), (1, 5, 6)])
    assert n_slabs == 0 and parsed == [({}, []), ({}, [])]
    write_sorted_input(tmp_path / "norecords.bam", REFS, [])
    check(engine, tmp_path / "norecords.bam", tmp_path / "norecords.kept.bam", 0)


def _small_array(stream, n):
    """``kept_index`` with room for one run fewer than the slab has."""
    import ctypes
    from mapdamage_amd.bai import RUN_DTYPE
    from mapdamage_amd.engine import MdxError
    runs = np.zeros(n, RUN_DTYPE)
    tid, pos, n_runs, bad, reason = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(0), ctypes.c_int64(-1), ctypes.c_int32(0)
    full, _ = stream.kept_index(0, (-1, -1), n)
    rc = stream._lib.mdx_gbam_kept_index(stream._g, ctypes.c_int64(0), ctypes.byref(tid), ctypes.byref(pos), ctypes.c_void_p(runs.ctypes.data),
                                         ctypes.c_int64(len(full) - 1), ctypes.byref(n_runs), ctypes.byref(bad), ctypes.byref(reason))
    if rc != 0:
        raise MdxError(rc, stream._error())


def test_refusals_on_the_command_line(sorted_data, tmp_path):
    """Unsorted input ends the run like a tag clash: exit code 1, the record's name and the reason, neither file; without the
    option the same input is written as before."""
    (tmp_path / "w").mkdir()
    out = run(sorted_data, tmp_path / "out", "unsorted.bam", "--write-kept", tmp_path / "w" / "kept.bam", "--write-index", rc=1)
    log = (out / "Runtime_log.txt").read_text()
    u = sorted_data["unsorted"]
    kept = np.flatnonzero((u.flag.astype(np.int64) & 0xF04) == 0)
    key = u.tid[kept].astype(np.int64) * (1 << 32) + u.pos[kept]
    first_bad = int(kept[1 + int(np.flatnonzero(np.diff(key) < 0)[0])])
    names = [r["name"] for r in Y.Bam(sorted_data["dir"] / "unsorted.bam").records]
    assert "Read: %s is to be written and lies in front of the written record before it" % names[first_bad] in log
    assert list((tmp_path / "w").iterdir()) == [] and not any((out / f).exists() for f in FILES + ("write_kept.tsv",))
    run(sorted_data, tmp_path / "out2", "unsorted.bam", "--write-kept", tmp_path / "w" / "kept.bam")
    assert sorted(p.name for p in (tmp_path / "w").iterdir()) == ["kept.bam"]
    # nothing written at all: both files, the index without bins
    out = run(sorted_data, tmp_path / "out3", "in.bam", "--min-read-length", "1000", "--write-kept", tmp_path / "w" / "none.bam", "--write-index")
    bam = Y.Bam(tmp_path / "w" / "none.bam")
    assert bam.records == [] and (tmp_path / "w" / "none.bam.bai").read_bytes() == Y.build_index(bam)
    assert "Wrote index %s.bai (0 references with records, 0 chunks)" % (tmp_path / "w" / "none.bam") in (out / "Runtime_log.txt").read_text()
