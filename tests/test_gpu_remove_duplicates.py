"""--remove-duplicates on the device (mapdamage_amd/csrc/mdx_dedup.hip): the flags ``mdx_dedup_mark`` leaves in the views of small
BAM files, the counters and the histogram against the brute force of tests/dup_rule.py — at the sizes where the kernels turn,
in one slab and in many, under contention, from a table of 8 slots —, and the command line against the same command on a file
without the duplicates.  The rule and the table on the host: tests/test_remove_duplicates.py."""

import dataclasses
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from tests import dup_rule as DR
from tests.test_gpu_strata import MIXED, genome5
from tests.test_gpu_write_kept import DEVICE, FILES, GOLDEN, RGS, LIBS, read_bam_file, run, tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
LIBS3 = [("s", "a"), ("s", "b"), ("t", "a")]
RG3 = ["rgA", "rgB", "rgC"]
HEADER_TEXT = ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n"
               + "".join("@RG\tID:%s\tSM:%s\tLB:%s\n" % (rg, s, l) for rg, (s, l) in zip(RG3, LIBS3)))
RAW_HEADER = (b"BAM\x01" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT.encode() + struct.pack("<i", 2)
              + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000000) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 500000))
UNKNOWN = 0xFFFF                             # the library of a record whose read group the stream was not told


def write_records(path, records, mapq=None):
    """``records``: (flag, lib, tid, pos, cigar) in file order; a library beyond the three gets a read group nobody knows."""
    bodies = [DR.body(f, t, p, c, rg=RG3[lib] if lib < 3 else "zz", salt=i, mapq=60 if mapq is None else int(mapq[i]))
              for i, (f, lib, t, p, c) in enumerate(records)]
    sam.write_bam_raw(str(path), RAW_HEADER, bodies)


def mark_file(eng, path, chunk_bytes=256 << 20, ends="both", begin=True, record_filter=None, drop=None):
    """Every slab of the file through ``dedup_mark``: the flag columns behind it, the slabs' sizes, counters, histogram, info.
    ``drop``: indices of records that get 0x200 in front of the mark, as the draws of -n 0.5 leave them."""
    if begin:
        eng.dedup_begin(ends)
    flags, slabs = [], []
    with sam.GpuBamStream(eng, str(path), readgroups=[(rg, i) for i, rg in enumerate(RG3)], chunk_bytes=chunk_bytes,
                          record_filter=record_filter) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                break
            if drop is not None:
                f = stream.view_flags(view)
                lo = sum(slabs)
                mine = drop[(drop >= lo) & (drop < lo + len(f))] - lo
                f[mine] |= 0x200
                stream.set_view_flags(view, f)
            eng.dedup_mark(view)
            flags.append(stream.view_flags(view))
            slabs.append(int(view.n_reads))
    eng.sync()
    return dict(flags=np.concatenate(flags) if flags else np.zeros(0, np.uint16), slabs=slabs, counts=eng.dedup_counts(),
                hist=eng.dedup_histogram(), info=eng.dedup_info())


def check(got, records, ends="both", n_libraries=3):
    """The flags are the file's with 0x400 on the brute force's duplicates and nowhere else; counters and histogram are its."""
    dup, counts, hist = DR.brute(records, n_libraries, ends)
    want = np.array([r[0] for r in records], np.int64) | np.where(dup, 0x400, 0)
    assert len(got["flags"]) == len(records)
    assert ((got["flags"].astype(np.int64) & 0xFFF) == (want & 0xFFF)).all(), np.flatnonzero((got["flags"].astype(np.int64) & 0xFFF) != (want & 0xFFF))[:10]
    assert (got["counts"] == counts).all(), (got["counts"], counts)
    assert (got["hist"] == hist).all()
    # examined = duplicates + molecules; the copies of the histogram are the examined records where no bin overflows
    assert (counts[:, 0] == counts[:, 1] + hist.sum(axis=1)).all()
    if not hist[:, -1].any():
        assert ((hist * np.arange(1, DR.BINS + 1, dtype=np.uint64)).sum(axis=1) == counts[:, 0]).all()
    assert got["info"]["examined"] == int(counts[:, 0].sum())
    return dup


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS3) as eng:
        yield eng


# ---------------------------------------------------------------------- 1. sizes where the kernels turn
def sized_records(n, kind):
    out = []
    for i in range(n):
        m = {"unique": i, "identical": 0, "halves": i % max(1, n // 2)}[kind]
        # (a molecule in its two spellings: `60M` at p, `5S55M` at p + 5)
        out.append((0x10 * (m % 2), m % 3, m % 2, 1000 + m + (5 if i % 2 else 0), [(S, 5), (M, 55)] if i % 2 else [(M, 60)]))
    return out


@pytest.fixture(scope="module")
def turns(engine):
    """The records a block of the stage's kernels takes (sign, compact, insert, lookup; rehash and histogram: slots), and those
    a round of the one-block scan takes — a count per lane of a larger block —, as the library tells them (``mdx_dedup_info``)."""
    engine.dedup_begin()
    info = engine.dedup_info()
    assert 64 <= info["block_records"] < info["scan_records"] <= 1 << 20
    return dict(block=info["block_records"], scan=info["scan_records"])


def sized(turns, size):
    """"65" -> 65; "block-1", "2*scan+1" -> in the units the library told."""
    return int(eval(size, {"__builtins__": {}}, dict(turns)))


@pytest.mark.parametrize("kind", ["unique", "identical", "halves"])
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "block-1", "block", "block+1", "2*block+1", "4*block+1"])
def test_sizes_where_the_kernels_turn(engine, turns, tmp_path, size, kind):
    n = sized(turns, size)
    records = sized_records(n, kind)
    write_records(tmp_path / "in.bam", records)
    dup = check(mark_file(engine, tmp_path / "in.bam"), records)
    assert dup.sum() == {"unique": 0, "identical": n - 1, "halves": n - max(1, n // 2)}[kind]


@pytest.fixture(scope="module")
def scan_rounds(turns):
    """One record more than a round of the scan takes, as short as records come (`4M`, or `1S3M` one base further on): seven
    records of ten are a molecule's only one, the others share 2 000 molecules, their copies in both rounds; one record of
    sixteen is not examined, so that the blocks' counts differ and a record's rank is not its index."""
    rng = np.random.default_rng(97)
    n = turns["scan"] + 1
    molecule = np.where(rng.random(n) < 0.7, 10_000 + np.arange(n), rng.integers(0, 2000, n))
    extra = np.where(rng.random(n) < 1 / 16, rng.choice((0x1, 0x400, 0x4), n), 0)
    clipped = rng.random(n) < 0.5
    records = [(0x10 * (m % 2) | e, m % 3, m % 2, 1000 + m + c, [(S, 1), (M, 3)] if c else [(M, 4)])
               for m, e, c in zip(molecule.tolist(), extra.tolist(), clipped.tolist())]
    bodies = [DR.body(f, t, p, c, rg=RG3[lib], salt=i) for i, (f, lib, t, p, c) in enumerate(records)]
    return dict(records=records, bodies=bodies)


@pytest.mark.parametrize("size", ["scan-1", "scan", "scan+1"])
def test_sizes_where_the_scan_turns(engine, turns, scan_rounds, tmp_path, size):
    """One slab of a round of the scan less one record, a round, and a round and a record: the last has a second round, which
    starts from the sum the first carried over — a wrong carry gives two records one ordinal, or a record an ordinal beyond
    the store, and the flags of the last block's records are no longer the brute force's."""
    n = sized(turns, size)
    records = scan_rounds["records"][:n]
    sam.write_bam_raw(str(tmp_path / "in.bam"), RAW_HEADER, scan_rounds["bodies"][:n])
    got = mark_file(engine, tmp_path / "in.bam")
    assert got["slabs"] == [n]
    dup = check(got, records)
    # (three records of ten share 2 000 molecules: nearly all of those are later copies, to the file's last records)
    assert n // 5 < dup.sum() < n // 3 and dup[-(n // 100):].any() and not dup[-(n // 100):].all()


# ---------------------------------------------------------------------- 2. the order of the file, not the slabs
def respell(rng, flag, lib, tid, left, span):
    """The molecule [left, left + span) in one of its spellings: clips at either end move pos and shorten the match."""
    lead = [[], [(S, 5)], [(H, 2), (S, 3)], [(H, 7)]][rng.integers(0, 4)]
    trail = [[], [(S, 4)], [(S, 1), (H, 5)]][rng.integers(0, 3)]
    a, b = sum(ln for _, ln in lead), sum(ln for _, ln in trail)
    core = [(M, span - a - b)] if rng.random() < 0.7 else [(M, 10), (D, 3), (EQ, span - a - b - 13)]
    return flag, lib, tid, left + a, lead + core + trail


@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    """20 000 records in three libraries, 30 % of them later copies in clusters of 2 to 50: a third of the copies right behind
    their first, the rest anywhere in the file — other slabs, in front of the first too."""
    rng = np.random.default_rng(41)
    n_total, n_dup = 20_000, 6_000
    sizes = []
    while sum(sizes) < n_dup:
        sizes.append(min(int(rng.integers(1, 50)), n_dup - sum(sizes)))         # copies beside the first
    n_mol = n_total - n_dup
    molecules = [(int(rng.choice((0, 0x10))), int(rng.integers(0, 3)), int(rng.integers(0, 2)), 100 + 7 * m + int(rng.integers(0, 7)),
                  int(rng.integers(40, 90))) for m in range(n_mol)]
    keyed = [(float(m), molecules[m]) for m in range(n_mol)]
    for c, size in enumerate(sizes):
        m = int(rng.integers(0, n_mol))
        for k in range(size):
            keyed.append((m + rng.random() if k % 3 == 0 else rng.random() * n_mol, molecules[m]))
    keyed.sort(key=lambda kv: kv[0])
    records = [respell(rng, *mol) for _, mol in keyed]
    # (some that are not examined, among them)
    for i in rng.choice(n_total, 600, replace=False):
        f, lib, t, p, c = records[i]
        records[i] = (f | int(rng.choice((0x1, 0x400, 0x100, 0x800, 0x4))), lib, t, p, c)
    d = tmp_path_factory.mktemp("clustered")
    write_records(d / "in.bam", records)
    write_records(d / "reversed.bam", records[::-1])
    return dict(dir=d, records=records)


@pytest.mark.parametrize("ends", ["both", "5p"])
@pytest.mark.parametrize("name", ["in.bam", "reversed.bam"])
def test_one_slab_and_many(engine, clustered, name, ends):
    records = clustered["records"] if name == "in.bam" else clustered["records"][::-1]
    one = mark_file(engine, clustered["dir"] / name, ends=ends)
    many = mark_file(engine, clustered["dir"] / name, 1 << 16, ends=ends)
    assert len(one["slabs"]) == 1 and len(many["slabs"]) >= 8
    dup = check(one, records, ends)
    check(many, records, ends)
    assert (one["flags"] == many["flags"]).all()
    assert 5_000 < dup.sum() < 8_000
    # a molecule's copies lie on both sides of a slab boundary
    slab_of = np.repeat(np.arange(len(many["slabs"])), many["slabs"])
    first = {}
    straddle = 0
    for i, r in enumerate(records):
        kind, sig = DR.signature(*r, 3, ends)
        if kind == DR.EXAMINED:
            straddle += slab_of[first.setdefault(sig, i)] != slab_of[i]
    assert straddle > 100


def test_the_representative_follows_the_order(clustered):
    """The reversed file keeps other copies: the test above compares two different answers.  (6 000 copies in clusters of at most
    50 are 120 clusters at least, and a cluster's first and last records change places.)"""
    a = DR.brute(clustered["records"], 3)[0]
    b = DR.brute(clustered["records"][::-1], 3)[0][::-1]
    assert a.sum() == b.sum() and (a != b).sum() > 2 * 120


# ---------------------------------------------------------------------- 3. contention
def test_one_molecule_twenty_thousand_times(engine, tmp_path):
    records = [(0, 1, 0, 500, [(M, 50)])] * 20_000
    write_records(tmp_path / "in.bam", records)
    got = mark_file(engine, tmp_path / "in.bam")
    assert len(got["slabs"]) == 1
    check(got, records)
    assert (got["flags"] & 0x400 != 0).tolist() == [False] + [True] * 19_999
    assert got["hist"][1, -1] == 1 and got["hist"].sum() == 1


def test_two_hundred_molecules_interleaved(engine, tmp_path):
    records = [(0x10 * (m % 2), m % 3, 0, 500 + m, [(M, 50)]) for _ in range(100) for m in range(200)]
    write_records(tmp_path / "in.bam", records)
    got = mark_file(engine, tmp_path / "in.bam")
    check(got, records)
    assert (got["flags"] & 0x400 != 0).tolist() == [False] * 200 + [True] * 19_800
    assert got["hist"][:, 99].sum() == 200 and got["hist"].sum() == 200


# ---------------------------------------------------------------------- 4. growth and walks
def test_from_a_table_of_eight_slots(clustered, tmp_path):
    prefix = str(tmp_path / "out")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_dedup_worker.py"), str(clustered["dir"] / "in.bam"), str(1 << 16),
                           "both", prefix], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_DUP_SLOTS="8"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    info = json.load(open(prefix + ".json"))
    dup = DR.brute(clustered["records"], 3)[0]
    assert ((np.load(prefix + ".npy") & 0x400 != 0) == (dup | np.array([r[0] & 0x400 != 0 for r in clustered["records"]]))).all()
    assert info["slabs"] >= 8 and info["growths"] >= 4 and info["slots"] >= 2 * info["examined"]


def test_consecutive_positions_of_a_sorted_file(engine, tmp_path):
    """What a coordinate-sorted file brings: runs of consecutive left ends under one tid.  At a load of at most 1/2 a walk of
    linear probing passes k slots with a probability that falls like (a e^(1 - a))^k = 0.824^k: among 10^4 inserts one of 120
    has a chance below 10^-6, and the mean of an insert is at most (1 + 1 / (1 - a)^2) / 2 = 2.5.  A hash that kept the
    neighbours together would walk hundreds."""
    records = [(0, 0, t, 1000 + i, [(M, 50)]) for t in (0, 1) for i in range(5000)]
    for i in (77, 5077, 9999):
        records.insert(i + 1, records[i])
    write_records(tmp_path / "in.bam", records)
    got = mark_file(engine, tmp_path / "in.bam", 1 << 16)
    assert check(got, records).sum() == 3
    info = got["info"]
    assert 2 * info["examined"] <= info["slots"]
    assert info["longest_probe"] <= 120 and info["probes"] <= 2.5 * info["examined"], info


# ---------------------------------------------------------------------- 5. what is not examined
def test_records_that_are_not_examined(engine, tmp_path):
    """Paired records that share every field, records the record filter or the draws dropped, 0x400 / 0x100 / 0x800 records, a
    library nobody knows: none is marked, none makes a later record a copy, and a dropped first copy does not shadow the second."""
    rng = np.random.default_rng(8)
    base = [(0x10 * (m % 2), m % 3, m % 2, 2000 + 3 * m, [(M, 40)]) for m in range(300)]
    records, mapq = [], []
    for rep in range(4):
        for m, (f, lib, t, p, c) in enumerate(base):
            what = (m + rep) % 8
            extra = {0: 0x1, 1: 0x400, 2: 0x100, 3: 0x800}.get(what, 0) if rep < 2 or what == 0 else 0
            records.append((f | extra, UNKNOWN if what == 4 and rep == 1 else lib, t, p, c))
            mapq.append(5 if what == 5 and rep == 0 else 60)                  # (--min-mapq 20 drops the first copy)
    write_records(tmp_path / "in.bam", records, mapq)
    drop = np.sort(rng.choice(len(records), 150, replace=False))
    got = mark_file(engine, tmp_path / "in.bam", 1 << 16, record_filter=sam.RecordFilter(min_mapq=20), drop=drop)
    seen = [(f | (0x200 if q < 20 or i in set(drop.tolist()) else 0), lib, t, p, c) for i, ((f, lib, t, p, c), q) in enumerate(zip(records, mapq))]
    dup = check(got, seen)
    assert not dup[[i for i, r in enumerate(seen) if r[0] & 0xF05 or r[1] == UNKNOWN]].any() and dup.sum() > 300
    counts = got["counts"].sum(axis=0)
    assert counts[2] > 100 and counts[3] == 0
    # the second copy of a molecule whose first copy the filter dropped is counted, the third is its copy
    m = next(m for m in range(300) if m % 8 == 5 and not {m, 300 + m, 600 + m} & set(drop.tolist()))
    assert [bool(got["flags"][k * 300 + m] & 0x400) for k in range(3)] == [False, False, True]


# ---------------------------------------------------------------------- 6. state
def test_reset_and_call_order(engine, tmp_path):
    from mapdamage_amd.engine import DamageEngine, MdxError
    records = sized_records(700, "halves")
    write_records(tmp_path / "in.bam", records)
    first = mark_file(engine, tmp_path / "in.bam")
    # the set goes on: the same records again are all copies
    again = mark_file(engine, tmp_path / "in.bam", begin=False)
    assert (again["flags"] & 0x400 != 0).all() and again["info"]["examined"] == 1400
    engine.reset()
    fresh = mark_file(engine, tmp_path / "in.bam", begin=False)
    assert (fresh["flags"] == first["flags"]).all() and (fresh["counts"] == first["counts"]).all() and (fresh["hist"] == first["hist"]).all()
    check(fresh, records)
    with DamageEngine(LIBS3) as other:
        with sam.GpuBamStream(other, str(tmp_path / "in.bam"), readgroups=[(rg, i) for i, rg in enumerate(RG3)]) as stream:
            with pytest.raises(MdxError) as error:
                other.dedup_mark(stream.next_view())
        assert error.value.code == -3 and "mdx_dedup_begin" in str(error.value)
        with pytest.raises(MdxError) as error:
            other.dedup_counts()
        assert error.value.code == -3


# ---------------------------------------------------------------------- 7. the command line: the contract of the record filters
@pytest.fixture(scope="module")
def dup_data(tmp_path_factory):
    """Records of the ``lib_data`` kind in coordinate order with planted copies (other MAPQ, other extra flag bits), and per
    value of --duplicate-ends the file a host script makes of it by deleting the brute force's duplicates."""
    d = tmp_path_factory.mktemp("dedup_cli")
    ref = genome5()
    rng = np.random.default_rng(2028)
    b = synth.make_reads(ref, 2000, 96, nlib=3, with_qual=True, **dict(MIXED, len_range=(30, 150)))
    index = np.concatenate([np.arange(b.n), rng.choice(b.n, 900)])
    index = index[np.lexsort((np.arange(len(index)), b.pos[index], b.tid[index]))]
    b = b.take(index)
    flag16 = b.flag.astype(np.int64)
    for bit in (0x1, 0x400, 0x800, 0x20):
        flag16 |= np.where(rng.random(b.n) < 0.06, bit, 0)
    b = dataclasses.replace(b, flag=flag16.astype(np.uint16))
    mapq = rng.choice((0, 24, 30, 37, 60), b.n)
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    fasta.write_fasta(d / "ref.fa", ref)
    off = b.cigar_off.astype(np.int64)
    records = [(int(flag16[i]), int(b.lib[i]), int(b.tid[i]), int(b.pos[i]), [(int(w) & 15, int(w) >> 4) for w in b.cigar[off[i]:off[i + 1]]])
               for i in range(b.n)]
    out = dict(dir=d, ref=ref, batch=b, records=records)
    header, file_records = read_bam_file(d / "in.bam")
    assert [struct.unpack_from("<iiBBHHH", r, 4)[::6] for r in file_records] == [(r[2], r[0]) for r in records]
    for ends in ("both", "5p"):
        dup, counts, hist = DR.brute(records, 3, ends)
        assert 300 < dup.sum() < 900
        # (the file's own records, byte for byte, without the duplicates)
        sam.write_bam_raw(str(d / ("without_%s.bam" % ends)), header, [r[4:] for r, gone in zip(file_records, dup) if not gone])
        out[ends] = (dup, counts, hist)
    assert (out["both"][0] != out["5p"][0]).any()
    return out


CONFIGS = {"plain": [], "by-reference": ["--by-reference"],
           "pipeline": ["--by-pmd-score", "--write-groups", "1", "--tag-group", "XG", "--mask-ends", "2,2", "--calmd", "--write-index"]}


@pytest.mark.parametrize("ends,config,route", [(e, c, "file") for e in ("both", "5p") for c in CONFIGS] + [("both", "pipeline", "pipe"), ("5p", "plain", "pipe")])
def test_command_line(dup_data, tmp_path, ends, config, route):
    opts = list(CONFIGS[config])
    kept, kept_plain = tmp_path / "kept.bam", tmp_path / "kept_plain.bam"
    with_option = run(dup_data, tmp_path / "with", "in.bam", "--remove-duplicates", *(["--duplicate-ends", ends] if ends != "both" else []),
                      *opts, *(["--write-kept", kept] if config != "by-reference" else []), route=route)
    without = run(dup_data, tmp_path / "without", "without_%s.bam" % ends, *opts, *(["--write-kept", kept_plain] if config != "by-reference" else []),
                  route=route)
    log = (with_option / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    assert tables(with_option) == tables(without)
    if config != "plain":
        by = "by_reference" if config == "by-reference" else "by_pmd"
        names = sorted(str(p.relative_to(without / by)) for p in (without / by).rglob("*") if p.is_file())
        assert names and names == sorted(str(p.relative_to(with_option / by)) for p in (with_option / by).rglob("*") if p.is_file())
        for name in names:
            assert (with_option / by / name).read_bytes() == (without / by / name).read_bytes(), name
    if config != "by-reference":
        assert read_bam_file(kept) == read_bam_file(kept_plain)
        assert (with_option / "write_kept.tsv").read_text().split("\t")[-2:] == (without / "write_kept.tsv").read_text().split("\t")[-2:]
    if config == "pipeline":
        # (the index speaks of the written file's blocks: byte for byte where both runs cut their input into the same slabs)
        if route == "file":
            assert open(str(kept) + ".bai", "rb").read() == open(str(kept_plain) + ".bai", "rb").read()
        for name in ("mask_ends.tsv", "calmd.tsv"):
            assert (with_option / name).read_text().split("\n")[1].split("\t")[1:] == (without / name).read_text().split("\n")[1].split("\t")[1:]
    # the option's own files and log line, against the brute force
    dup, counts, hist = dup_data[ends]
    rows = ["Sample\tLibrary\tExamined\tDuplicates\tMolecules\tPaired\tOther\n"]
    bins = ["Sample\tLibrary\tCopies\tMolecules\n"]
    for (sample, library), (e, d, p, o), h in zip(LIBS, counts.tolist(), hist.tolist()):
        rows.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (sample, library, e, d, e - d, p, o))
        bins += ["%s\t%s\t%d\t%d\n" % (sample, library, c + 1, m) for c, m in enumerate(h) if m]
    assert (with_option / "duplicates.tsv").read_text() == "".join(rows)
    assert (with_option / "duplicates_histogram.tsv").read_text() == "".join(bins)
    e, d, p, o = (int(x) for x in counts.sum(axis=0))
    assert "Duplicates: %d records examined, %d removed, %d molecules; not examined: %d paired, %d other" % (e, d, e - d, p, o) in log
    assert p > 0 and "paired records were not examined" in log
    # without the option: neither file, no line
    assert not (without / "duplicates.tsv").exists() and not (without / "duplicates_histogram.tsv").exists()
    assert "Duplicates:" not in (without / "Runtime_log.txt").read_text()


def test_many_slabs_on_the_command_line(dup_data, tmp_path, monkeypatch):
    """The same tables from slabs of 64 KiB, with a grouping and the filters on top."""
    opts = ["--by-terminal-damage", "--min-mapq", "25", "--merge-libraries"]
    one = run(dup_data, tmp_path / "one", "in.bam", "--remove-duplicates", *opts)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    many = run(dup_data, tmp_path / "many", "in.bam", "--remove-duplicates", *opts)
    assert tables(one) == tables(many)
    assert (one / "duplicates.tsv").read_text() == (many / "duplicates.tsv").read_text()
    # (merged libraries: one row, and the filter's records are in none of its columns)
    rows = (one / "duplicates.tsv").read_text().splitlines()
    assert len(rows) == 2 and rows[1].startswith("*\t*\t")
    seen = [(f | (0x200 if q < 25 else 0), 0, t, p, c) for (f, _, t, p, c), q in zip(dup_data["records"], _mapq(dup_data))]
    dup, counts, _ = DR.brute(seen, 1)
    assert rows[1].split("\t")[2:] == [str(int(x)) for x in (counts[0, 0], counts[0, 1], counts[0, 0] - counts[0, 1], counts[0, 2], counts[0, 3])]


def test_the_last_bin_on_the_command_line(dup_data, tmp_path):
    """A molecule of 1 100 copies and one of exactly 1 024 are written `>=1024`, one of 1 023 by its number."""
    b, ref, records = dup_data["batch"], dup_data["ref"], dup_data["records"]
    examined = [i for i, r in enumerate(records) if DR.signature(*r, 3)[0] == DR.EXAMINED]
    firsts = {}
    for i in examined:
        firsts.setdefault(DR.signature(*records[i], 3)[1], i)
    a, c, e = [i for i in firsts.values() if i >= 60][:3]         # (none of the 60 records in front is one of theirs)
    index = np.sort(np.array(list(range(60)) + [a] * 1100 + [c] * 1024 + [e] * 1023))
    rows = [records[i] for i in index]
    sam.write_bam(str(tmp_path / "in.bam"), b.take(index), ref.names, ref.lengths, RGS, [RGS[r[1]]["ID"] for r in rows])
    out = run(dup_data, tmp_path / "out", tmp_path / "in.bam", "--remove-duplicates")
    dup, counts, hist = DR.brute(rows, 3)
    assert hist[:, -1].sum() == 2 and hist[:, -2].sum() == 1 and dup.sum() >= 1099 + 1023 + 1022
    bins = ["Sample\tLibrary\tCopies\tMolecules\n"]
    for (sample, library), h in zip(LIBS, hist.tolist()):
        bins += ["%s\t%s\t%s\t%d\n" % (sample, library, ">=1024" if copies == 1024 else "%d" % copies, m) for copies, m in enumerate(h, 1) if m]
    text = (out / "duplicates_histogram.tsv").read_text()
    assert text == "".join(bins)
    assert text.count("\t>=1024\t") == len({records[i][1] for i in (a, c)}) and "\t1023\t1\n" in text and "\t1024\t" not in text
    total = counts.sum(axis=0)
    assert "Duplicates: %d records examined, %d removed, %d molecules" % (total[0], total[1], total[0] - total[1]) in (out / "Runtime_log.txt").read_text()


def _mapq(dup_data):
    return [r[13] for r in read_bam_file(dup_data["dir"] / "in.bam")[1]]


# ---------------------------------------------------------------------- 8. refusals at run time
def test_sam_text_is_refused(dup_data, tmp_path):
    b, ref = dup_data["batch"].slice(0, 200), dup_data["ref"]
    sam.write_sam(str(tmp_path / "in.sam"), b, ref.names, ref.lengths, RGS, [RGS[int(i)]["ID"] for i in b.lib])
    out = run(dup_data, tmp_path / "sam", tmp_path / "in.sam", "--remove-duplicates", rc=1)
    assert "--remove-duplicates needs BAM input" in (out / "Runtime_log.txt").read_text()
    assert not any((out / f).exists() for f in FILES + ("duplicates.tsv", "duplicates_histogram.tsv"))


def test_a_file_the_device_path_gives_up_on_ends_the_run(tmp_path):
    from mapdamage_amd.main import main
    from tests.test_foreign_bam import reference, truth
    fasta.write_fasta(tmp_path / "ref.fa", reference(truth("full")[1]))
    out = tmp_path / "out"
    assert main(["-i", os.path.join(GOLDEN, "foreign.bam"), "-r", str(tmp_path / "ref.fa"), "-d", str(out), "--no-stats", "--remove-duplicates"]) == 1
    log = (out / "Runtime_log.txt").read_text()
    assert "GPU decode path gave up" in log and "CG tag" in log
    assert "--remove-duplicates marks the records on the device decode path" in log.split("GPU decode path gave up")[1]
    assert not any((out / f).exists() for f in FILES + ("duplicates.tsv", "duplicates_histogram.tsv"))
