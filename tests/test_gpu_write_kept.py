"""--write-kept on the GPU (include/mdx.h ``mdx_gbam_kept_bound`` / ``mdx_gbam_write_kept``; csrc/mdx_kept.h): the records a
run counted, or those of chosen groups, selected, compacted and compressed on the device.

The yardstick shares nothing with the product: ``read_bam_file`` below checks every BGZF member of a file (magic, BC
subfield, BSIZE, and ``zlib.decompress(member, 31)``: CRC32 and ISIZE), the end-of-file marker, and splits the inflated
stream into header and records by block_size.  The expectation is ``[record for record, keep in zip(input, predicate) if
keep]``: the input records are the bytes ``encode`` below made (tests 1 to 4) or what the same reader finds in the input file
(tests 5 to 7), the predicate is numpy over the columns the test made.

The scan's constants, beside the kernels' (csrc/mdx_gbam.hip): KEPT_TILE records per tile of the first and third launch,
KEPT_SCAN_ROUND tiles per round of the one block of the second, KEPT_WAVE_BYTES above which a record is copied by a whole
wavefront instead of eight lanes."""

import dataclasses
import functools
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from tests import damage_util as D
from tests import pmd_util as P
from tests import regions_util as R
from tests.test_gpu_pipe_input import _main_on_pipe
from tests.test_gpu_record_filters import ARGS, FILTERS
from tests.test_gpu_strata import MIXED, genome5

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEPT_TILE, KEPT_SCAN_ROUND, KEPT_WAVE_BYTES = 256, 256, 4096
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
DROP_BITS = (0x4, 0x100, 0x200, 0x400, 0x800)
FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")
DEVICE = "Decode path: device; fallbacks from the device path: 0"
HEADER_TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n@RG\tID:rgA\tSM:s\tLB:l\n"
RAW_HEADER = (b"BAM\x01" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT.encode() + struct.pack("<i", 2)
              + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000000) + struct.pack("<i", 5) + b"chr2\0" + struct.pack("<i", 500000))
POOL = np.random.default_rng(11).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------- the yardstick: a reader of its own
def bgzf_members(data, marker=True):
    """The inflated bytes of a BGZF file, every member checked, the end-of-file marker too (``marker=False``: an input of
    another writer's, which may end without one)."""
    assert not marker or data[-28:] == EOF_MARKER
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 12] == b"\x06\x00" and data[at + 12:at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + size <= len(data)
        out.append(zlib.decompress(data[at:at + size], 31))          # (CRC32 and ISIZE are zlib's to check)
        assert len(out[-1]) <= 65536
        at += size
    assert at == len(data) and (not marker or out[-1] == b"")
    return b"".join(out)


def split_stream(stream, at=0):
    records = []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        assert size >= 32 and at + 4 + size <= len(stream)
        records.append(stream[at:at + 4 + size])
        at += 4 + size
    assert at == len(stream)
    return records


def read_bam_file(path, marker=True):
    """(header bytes, records with their block_size fields) of a BAM file."""
    stream = bgzf_members(open(path, "rb").read(), marker)
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    return stream[:at], split_stream(stream, at)


def members_stream(members):
    """The inflated bytes of the members ``write_kept`` returned (no header, no marker)."""
    data = bytes(members)
    return bgzf_members(data + EOF_MARKER) if data else b""


# ---------------------------------------------------------------------- the encoder
def encode(i, flag=0, n_bases=None, tag=None, name_len=None, z_bytes=0):
    """Record ``i`` without its block_size: names cycle through l_read_name 1 to 32, sequences through 0 to 200 bases, tags
    through none, RG:Z, a B:i array and a long XA:Z."""
    name_len = 1 + i % 32 if name_len is None else name_len
    n_bases = (i * 7) % 201 if n_bases is None else n_bases
    tag = i % 4 if tag is None else tag
    o = (i * 977) % (len(POOL) - 700_000)
    name = bytes(33 + b % 90 for b in POOL[o:o + name_len - 1]) + b"\0"
    cigar = struct.pack("<I", n_bases << 4) if n_bases else b""
    body = struct.pack("<iiBBHHHiiii", i % 2, 100 + i % 400_000, name_len, i % 61, 4680, len(cigar) // 4, flag, n_bases, -1, -1, 0)
    body += name + cigar + POOL[o + 40:o + 40 + (n_bases + 1) // 2] + bytes(b & 0x3F for b in POOL[o + 200:o + 200 + n_bases])
    if tag == 1:
        body += b"RGZrgA\0"
    elif tag == 2:
        k = i % 9
        body += b"ZBBi" + struct.pack("<i", k) + POOL[o:o + 4 * k]
    elif tag == 3:
        body += b"XAZ" + bytes(33 + b % 90 for b in POOL[o + 300:o + 400 + i % 50]) + b"\0"
    if z_bytes:
        body += b"ZZZ" + bytes(33 + b % 90 for b in POOL[o:o + z_bytes]) + b"\0"
    return body


def minimal(i, flag=0):
    """37 to 40 bytes with the block_size: no bases, no operations, no tags, a name of 0 to 3 characters."""
    return encode(i, flag, n_bases=0, tag=0, name_len=1 + i % 4)


def with_flag(body, flag):
    return body[:14] + struct.pack("<H", flag) + body[16:]


def flags_of(keep, base=None):
    """The pattern as flags: a dropped record gets one of the five bits of 0xF04, in turn; the bits that drop nothing vary."""
    n = len(keep)
    flag = (np.arange(n) % 2 * 0x10 + np.arange(n) % 3 // 2 * 0x1).astype(np.int64) if base is None else base.astype(np.int64)
    dropped = np.flatnonzero(~keep)
    flag[dropped] |= np.asarray(DROP_BITS)[np.arange(len(dropped)) % 5]
    return flag


def patterns(n):
    idx = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "every other": idx % 2 == 0, "first": idx == 0,
            "last": idx == n - 1, "coin": np.random.default_rng(n + 1).random(n) < 0.5}


def write_bgzf(path, data, block_bytes, level=6):
    """The other layout: blocks of ``block_bytes`` inflated bytes whatever the record boundaries."""
    with open(path, "wb") as out:
        for lo in range(0, len(data), block_bytes):
            chunk = data[lo:lo + block_bytes]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = c.compress(chunk) + c.flush()
            out.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body
                      + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        out.write(EOF_MARKER)


def write_input(path, bodies, layout):
    if layout == "raw":
        sam.write_bam_raw(str(path), RAW_HEADER, bodies)
    else:
        write_bgzf(path, RAW_HEADER + b"".join(struct.pack("<i", len(b)) + b for b in bodies), 3001)


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("s", "l")]) as eng:
        yield eng


def open_stream(eng, path, chunk_bytes=256 << 20, **kw):
    return sam.GpuBamStream(eng, str(path), readgroups=[("rgA", 0)], lib_default=0, chunk_bytes=chunk_bytes, **kw)


def kept_of_file(eng, path, chunk_bytes=256 << 20):
    """Every slab's ``write_kept``: (inflated streams per slab, records written, raw bytes)."""
    streams, n_written, raw = [], 0, 0
    with open_stream(eng, path, chunk_bytes) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                break
            bound = stream.kept_bound()
            members, n, r = stream.write_kept(view)
            assert len(members) <= bound
            streams.append(members_stream(members))
            assert len(streams[-1]) == r and (n == 0) == (len(members) == 0)
            assert len(split_stream(streams[-1])) == n
            n_written += n
            raw += r
    return streams, n_written, raw


def check_file(eng, path, bodies, keep, chunk_bytes=256 << 20):
    want = [struct.pack("<i", len(b)) + b for b, k in zip(bodies, keep) if k]
    streams, n_written, raw = kept_of_file(eng, path, chunk_bytes)
    got = b"".join(streams)
    assert n_written == len(want) and raw == sum(len(w) for w in want)
    assert got == b"".join(want)
    assert split_stream(got) == want
    return streams


# ---------------------------------------------------------------------- 1. sizes where the kernels turn
@functools.lru_cache(maxsize=None)
def plain_bodies(small):
    """Record bodies with flag 0, shared by the cases: the full cycle of shapes, or (the sizes of tens of thousands) shapes
    of 0 to 20 bases."""
    return [encode(i, 0, n_bases=i % 21) if small else encode(i) for i in range(KEPT_TILE * KEPT_SCAN_ROUND + 1 if small else 4097)]


SIZES = [0, 1, 2, 63, 64, 65, KEPT_TILE - 1, KEPT_TILE, KEPT_TILE + 1, 1023, 1024, 1025, 4097,
         KEPT_TILE * KEPT_SCAN_ROUND - 1, KEPT_TILE * KEPT_SCAN_ROUND, KEPT_TILE * KEPT_SCAN_ROUND + 1]


@pytest.mark.parametrize("layout", ["raw", "3001"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_where_the_kernels_turn(engine, tmp_path, n, layout):
    if layout == "3001" and n > 4097:
        layout = "30011"            # (the same layout in larger blocks: twenty thousand BGZF blocks of 3001 bytes take seconds to write)
    plain = plain_bodies(n > 4097)[:n]
    sizes = {(len(b) + 4) % 16 for b in plain}
    assert n < 1024 or sizes == set(range(16))
    for name, keep in patterns(n).items():
        flag = flags_of(keep)
        bodies = [with_flag(b, int(f)) for b, f in zip(plain, flag)]
        path = tmp_path / ("%s.bam" % name.replace(" ", "_"))
        if layout == "30011":
            write_bgzf(path, RAW_HEADER + b"".join(struct.pack("<i", len(b)) + b for b in bodies), 30011, level=1)
        else:
            write_input(path, bodies, layout)
        if n <= 4097:       # (the test's own writers against its own reader)
            assert read_bam_file(path) == (RAW_HEADER, [struct.pack("<i", len(b)) + b for b in bodies])
        check_file(engine, path, bodies, keep)


# ---------------------------------------------------------------------- 2. many slabs
@pytest.mark.parametrize("layout", ["raw", "3001"])
def test_many_slabs(engine, tmp_path, layout):
    n = 7000
    keep = np.random.default_rng(3).random(n) < 0.6
    keep[1200:3400] = False                 # a stretch of dropped records longer than two slabs
    keep[3400:3500] = True
    bodies = [encode(i, int(f)) for i, f in enumerate(flags_of(keep))]
    path = tmp_path / "in.bam"
    write_input(path, bodies, layout)
    assert 800_000 < os.path.getsize(path) < 1_800_000
    streams = check_file(engine, path, bodies, keep, chunk_bytes=65536)
    assert len(streams) >= 12
    # the emptied slabs contribute nothing; those around them something
    assert sum(1 for s in streams if not s) >= 2 and streams[0] and streams[-1]


# ---------------------------------------------------------------------- 3. long records
@pytest.mark.parametrize("where", ["start", "middle", "last"])
@pytest.mark.parametrize("what", ["70000 bases", "300000-byte tag"])
@pytest.mark.parametrize("long_kept", [True, False])
def test_long_records(engine, tmp_path, what, where, long_kept):
    long_body = encode(5, n_bases=70_000, tag=1) if what == "70000 bases" else encode(6, n_bases=50, tag=2, z_bytes=300_000)
    assert len(long_body) > (100_000 if what == "70000 bases" else 300_000)
    short = [minimal(i) for i in range(41)]
    assert {len(b) + 4 for b in short} == {37, 38, 39, 40}
    at = {"start": 0, "middle": 20, "last": 41}[where]
    plain = short[:at] + [long_body] + short[at:]
    keep = np.arange(len(plain)) % 2 == (at % 2 if long_kept else 1 - at % 2)       # neighbours kept and dropped alternately
    assert bool(keep[at]) == long_kept
    bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep))]
    for layout in ("raw", "3001"):
        path = tmp_path / (layout + ".bam")
        write_input(path, bodies, layout)
        check_file(engine, path, bodies, keep)
    # ... and both neighbours kept around a dropped long record, and the reverse
    keep2 = ~keep
    keep2[at] = keep[at]
    bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep2))]
    write_input(tmp_path / "second.bam", bodies, "raw")
    check_file(engine, tmp_path / "second.bam", bodies, keep2)


def test_records_around_the_wavefront_threshold(engine, tmp_path):
    """Records of KEPT_WAVE_BYTES - 1, KEPT_WAVE_BYTES and KEPT_WAVE_BYTES + 1 bytes (eight lanes, eight lanes, a wavefront), and
    several long ones in one wavefront's eight records."""
    plain = []
    for k, size in enumerate([KEPT_WAVE_BYTES - 1, KEPT_WAVE_BYTES, KEPT_WAVE_BYTES + 1, 3 * KEPT_WAVE_BYTES + 5] * 4):
        base = len(encode(k, n_bases=0, tag=0, name_len=2)) + 4 + 4
        plain += [encode(k, n_bases=0, tag=0, name_len=2, z_bytes=size - base), minimal(k)]
        assert len(plain[-2]) + 4 == size
    keep = np.random.default_rng(9).random(len(plain)) < 0.7
    bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep))]
    write_input(tmp_path / "in.bam", bodies, "raw")
    check_file(engine, tmp_path / "in.bam", bodies, keep)
    keep[:] = True
    bodies = [with_flag(b, 0) for b in plain]
    write_input(tmp_path / "all.bam", bodies, "raw")
    check_file(engine, tmp_path / "all.bam", bodies, keep)


# ---------------------------------------------------------------------- 4. scan depth
def test_scan_depth(engine, tmp_path):
    """300 000 minimal records in one slab: 1172 tiles, five rounds of the second launch's one block."""
    n = 300_000
    assert n > 4 * KEPT_TILE * KEPT_SCAN_ROUND
    keep = np.random.default_rng(4).random(n) < 0.5
    flag = flags_of(keep)
    variants = {}
    bodies = []
    for i in range(n):
        key = (i % 8, int(flag[i]))
        if key not in variants:
            variants[key] = minimal(i % 8, int(flag[i]))
        bodies.append(variants[key])
    path = tmp_path / "in.bam"
    sam.write_bam_raw(str(path), RAW_HEADER, bodies)
    streams = check_file(engine, path, bodies, keep)
    assert len(streams) == 1 and len(streams[0]) > 5_000_000


# ---------------------------------------------------------------------- 5. groups, all four kinds, at the library level
RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s1", "LB": "lib2"}, {"ID": "c", "SM": "s2", "LB": "lib1"}]
LIBS = [("s1", "lib1"), ("s1", "lib2"), ("s2", "lib1")]
THRESHOLDS = (-1.0, 1.0, 3.0)
GROUP_OF_TID = [0, 1, 2, 1, 0]


@pytest.fixture(scope="module")
def lib_data(tmp_path_factory):
    """A few thousand records over genome5() in three libraries, with qualities, MAPQ and extra flag bits; as BAM in both
    layouts; the input records as the reader above finds them; every kind of group of every record by the yardsticks."""
    d = tmp_path_factory.mktemp("write_kept")
    ref = genome5()
    rng = np.random.default_rng(2026)
    b = synth.make_reads(ref, 3000, 93, nlib=3, with_qual=True, **dict(MIXED, len_range=(30, 150)))
    nb = b.seq.shape[0]
    b.qual = np.where(rng.random(nb) < 0.05, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    n = b.n
    flag16 = b.flag.astype(np.int64)
    for bit in (0x1, 0x400, 0x800):
        flag16 |= np.where(rng.random(n) < 0.1, bit, 0)
    mapq = rng.choice((0, 1, 24, 25, 29, 30, 37, 60, 255), n)
    mapq[1000:1900] = rng.choice((0, 1, 24), 900)         # whole slabs of 64 KiB that --min-mapq 25 empties
    b = dataclasses.replace(b, flag=flag16.astype(np.uint16))
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), b, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    sam.write_bam(str(d / "straddle.bam"), b, ref.names, ref.lengths, RGS, rg, mapq=mapq, htslib_blocks=False, block_bytes=3001)
    fasta.write_fasta(d / "ref.fa", ref)
    header, records = read_bam_file(d / "in.bam")
    assert read_bam_file(d / "straddle.bam") == (header, records) and len(records) == n
    # (the columns the predicate reads are the file's: flag and MAPQ of every record as the reader finds them)
    assert [struct.unpack_from("<H", r, 18)[0] for r in records] == flag16.tolist() and [r[13] for r in records] == mapq.tolist()
    regions = R.grid_regions()
    (d / "panels.bed").write_text(R.bed_text(regions, ref.names, R.GRID_GROUPS))
    S = P.scores(ref, b)
    groups = {"pmd": P.groups_of(S, THRESHOLDS), "pmd3": P.groups_of(S, (3.0,)), "regions": R.brute_group(b, regions, 5, 3),
              "damage": D.groups_of(D.first_damage(ref, b, LIBS, 0), 1), "reference": np.asarray(GROUP_OF_TID)[b.tid]}
    for kind, n_groups in (("pmd", 4), ("regions", 4), ("damage", 4), ("reference", 3)):
        assert (np.bincount(groups[kind], minlength=n_groups) >= 5).all(), kind
    kept = (flag16 & 0xF04) == 0
    assert 0 < kept.sum() < n
    return dict(dir=d, ref=ref, batch=b, flag16=flag16, mapq=mapq, lens=np.diff(b.seq_off.astype(np.int64)), header=header,
                records=records, groups=groups, kept=kept, regions=regions)


def strata_engine(kind, ref):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_regions import columns
    names = {"pmd": ["a", "b", "c", "d"], "regions": R.GRID_GROUPS, "damage": D.GROUPS, "reference": ["x", "y", "z"]}[kind]
    eng = DamageEngine(LIBS, 70, 10, 0, groups=names)
    try:
        if kind == "pmd":
            eng.set_strata_pmd(THRESHOLDS)
        elif kind == "regions":
            eng.set_strata_regions(*columns(R.grid_regions(), 5))
        elif kind == "damage":
            eng.set_strata_damage(1)
        else:
            eng.set_strata(GROUP_OF_TID)
        eng.set_reference(ref)
    except Exception:
        eng.close()
        raise
    return eng, len(names)


def lib_stream(eng, path, kind, chunk_bytes=1 << 16):
    return sam.GpuBamStream(eng, str(path), readgroups=[(r["ID"], LIBS.index((r["SM"], r["LB"]))) for r in RGS], chunk_bytes=chunk_bytes,
                            want_qual=kind == "pmd", packed=True if kind == "pmd" else None)


@pytest.mark.parametrize("source", ["in.bam", "straddle.bam"])
@pytest.mark.parametrize("kind", ["pmd", "regions", "damage", "reference"])
def test_groups_at_the_library_level(lib_data, kind, source):
    eng, n_groups = strata_engine(kind, lib_data["ref"])
    selections = [(1,), (0, n_groups - 1), tuple(range(n_groups)), None]
    got = {s: [] for s in selections}
    counts = {s: 0 for s in selections}
    with eng:
        with lib_stream(eng, lib_data["dir"] / source, kind) as stream:
            n_views = 0
            while True:
                view = stream.next_view()
                if view is None:
                    break
                n_views += 1
                eng.tabulate_view(view)
                for s in selections:
                    members, n, raw = stream.write_kept(view, s, n_groups if s is not None else 0)
                    got[s].append(members_stream(members))
                    counts[s] += n
                    assert raw == len(got[s][-1])
            eng.sync()
            assert n_views >= 5
    group = lib_data["groups"][kind]
    for s in selections:
        keep = lib_data["kept"] & (np.isin(group, s) if s is not None else True)
        want = [r for r, k in zip(lib_data["records"], keep) if k]
        assert counts[s] == len(want) and 0 < len(want)
        assert b"".join(got[s]) == b"".join(want), s
    assert got[selections[2]] == got[None]
    assert 0 < counts[(1,)] < counts[(0, n_groups - 1)] + counts[(1,)] <= counts[None]


def test_group_state_errors(lib_data):
    from mapdamage_amd.engine import DamageEngine, MdxError
    eng, n_groups = strata_engine("reference", lib_data["ref"])
    with eng:
        with lib_stream(eng, lib_data["dir"] / "in.bam", "reference") as stream:
            view = stream.next_view()
            with pytest.raises(MdxError, match="tabulate the view first") as err:         # before the view is tabulated
                stream.write_kept(view, (0,), n_groups)
            assert err.value.code == -3
            assert stream.write_kept(view)[1] > 0                                          # (no selection: no key needed)
            eng.tabulate_view(view)
            with pytest.raises(MdxError, match="n_groups 4, the context has 3") as err:    # a wrong n_groups
                stream.write_kept(view, (0,), n_groups + 1)
            assert err.value.code == -1
            first = stream.write_kept(view, (0,), n_groups)
            assert first[1] > 0
            first = (bytes(first[0]), first[1], first[2])
            # another batch tabulated in between
            eng.tabulate(lib_data["batch"].slice(0, 100))
            eng.sync()
            with pytest.raises(MdxError, match="not that of this view") as err:
                stream.write_kept(view, (0,), n_groups)
            assert err.value.code == -3
            # the next view, not tabulated yet, behind a tabulated one
            view = stream.next_view()
            with pytest.raises(MdxError) as err:
                stream.write_kept(view, (0,), n_groups)
            assert err.value.code == -3
            eng.tabulate_view(view)
            assert stream.write_kept(view, (0,), n_groups)[1] > 0
            eng.sync()
    with DamageEngine(LIBS) as plain:                                                     # a selection on an unstratified context
        plain.set_reference(lib_data["ref"])
        with lib_stream(plain, lib_data["dir"] / "in.bam", "reference") as stream:
            view = stream.next_view()
            plain.tabulate_view(view)
            with pytest.raises(MdxError, match="without strata") as err:
                stream.write_kept(view, (0,), 3)
            assert err.value.code == -1
            plain.sync()


# ---------------------------------------------------------------------- 6. the command line
def run(lib_data, out, source, *args, route="file", rc=0, env=None):
    from mapdamage_amd.main import main
    base = ["-r", str(lib_data["dir"] / "ref.fa"), "-d", str(out), "--log-level", "DEBUG", "--no-stats"] + [str(a) for a in args]
    source = source if os.path.isabs(str(source)) else lib_data["dir"] / source
    if route == "pipe":
        assert _main_on_pipe(out.parent, open(source, "rb").read(), base, "fifo", seed=zlib.crc32(str(out).encode()) % 10_000) == rc
    elif route == "stdin":
        with open(source, "rb") as handle:
            done = subprocess.run([sys.executable, "-m", "mapdamage_amd", "-i", "-"] + base, stdin=handle, cwd=ROOT,
                                  env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, timeout=300)
        assert done.returncode == rc, done.stderr.decode()[-2000:]
    else:
        assert main(["-i", str(source)] + base) == rc
    return out


def tables(folder):
    return [(folder / f).read_text() for f in FILES]


def group_rows(path):
    rows = [line.split("\t") for line in path.read_text().splitlines()[1:]]
    return {r[1]: (int(r[0]), int(r[-1])) for r in rows}


def cli_predicate(lib_data, option):
    """(options, predicate or None, the by_* directory and group name of the selection or None)."""
    q, req, exc, lo, hi = FILTERS["all"]
    f, kept = lib_data["flag16"], lib_data["kept"]
    passes = ((f & req) == req) & ((f & exc) == 0) & (lib_data["mapq"] >= q) & (lib_data["lens"] >= lo) & (lib_data["lens"] <= hi)
    if option == "a":
        return ARGS["all"], kept & passes, None
    if option == "b":
        return ARGS["all"] + ["--downsample", "0.5", "--downsample-seed", "7"], None, None
    if option == "c":
        return ["--by-pmd-score", "--write-groups", "1"], kept & (lib_data["groups"]["pmd3"] == 1), ("by_pmd", ">=3")
    return (["--region-groups", lib_data["dir"] / "panels.bed", "--write-groups", "0"],
            kept & (lib_data["groups"]["regions"] == R.GRID_GROUPS.index(first_group(lib_data))), ("by_region", first_group(lib_data)))


def first_group(lib_data):
    """The group --region-groups numbers 0: the first one the BED file names."""
    return R.GRID_GROUPS[lib_data["regions"][0][3]]


@pytest.fixture(scope="module")
def without_option(lib_data, tmp_path_factory):
    """The same command without --write-kept (and --write-groups), once per set of options."""
    done = {}

    def get(option):
        if option not in done:
            opts = [a for a in cli_predicate(lib_data, option)[0]]
            if "--write-groups" in opts:
                del opts[opts.index("--write-groups"):opts.index("--write-groups") + 2]
            done[option] = run(lib_data, tmp_path_factory.mktemp("plain_" + option) / "out", "in.bam", *opts)
            assert not (done[option] / "write_kept.tsv").exists()
        return done[option]
    return get


# (stdin proper needs a process of its own, started cold: once, with the filters; a named pipe carries the other options)
@pytest.mark.parametrize("option,route", [(o, r) for o in "abcd" for r in ("file", "straddle", "pipe", "slabs")] + [("a", "stdin")])
def test_command_line(lib_data, without_option, tmp_path, monkeypatch, option, route):
    if route == "slabs":
        monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    opts, predicate, selection = cli_predicate(lib_data, option)
    kept_path = tmp_path / "kept.bam"
    out = run(lib_data, tmp_path / "out", "straddle.bam" if route == "straddle" else "in.bam", *opts, "--write-kept", kept_path,
              route=route if route in ("pipe", "stdin") else "file")
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["kept.bam"]          # no temporary file is left
    header, records = read_bam_file(kept_path)
    assert header == lib_data["header"]
    if predicate is not None:
        assert 100 < predicate.sum() < lib_data["kept"].sum()
        assert records == [r for r, k in zip(lib_data["records"], predicate) if k]
    # the log line and write_kept.tsv against groups.tsv / the kept count
    which = "all" if selection is None else opts[opts.index("--write-groups") + 1]
    assert "Wrote %d records to %s (groups: %s)" % (len(records), kept_path, which) in log
    assert (out / "write_kept.tsv").read_text() == "path\tgroups\trecords\tuncompressed_bytes\n%s\t%s\t%d\t%d\n" % (
        kept_path, which, len(records), sum(len(r) for r in records))
    if selection is None:
        lines = [line for line in log.splitlines() if "filtered alignments processed" in line]
        assert len(lines) == 1 and "Done. %d filtered alignments processed" % len(records) in lines[0]
        want_folder = out
    else:
        index, reads = group_rows(out / selection[0] / "groups.tsv")[selection[1]]
        assert index == int(which) and reads == len(records)
        want_folder = out / selection[0] / str(index)
    # the usual files are those of the run without the option
    assert tables(out) == tables(without_option(option))
    # round trip: the plain command on the written file counts what the first run counted (or its group did)
    monkeypatch.delenv("MDX_GBAM_SLAB_BYTES", raising=False)
    again = run(lib_data, tmp_path / "again", kept_path)
    assert tables(again) == tables(want_folder)
    assert DEVICE in (again / "Runtime_log.txt").read_text()


# ---------------------------------------------------------------------- 7. other writers' files
@pytest.mark.parametrize("name,extra", [("foreign_nocg.bam", []), ("foreign_nolb.bam", ["--merge-libraries"])])
def test_other_writers_files(tmp_path, name, extra):
    from mapdamage_amd.main import main
    from tests.test_foreign_bam import reference, truth
    fasta.write_fasta(tmp_path / "ref.fa", reference(truth("nocg")[1]))
    header, records = read_bam_file(os.path.join(GOLDEN, name), marker=False)
    kept = [r for r in records if not struct.unpack_from("<H", r, 18)[0] & 0xF04]
    assert 0 < len(kept) <= len(records)
    out = tmp_path / "out"
    assert main(["-i", os.path.join(GOLDEN, name), "-r", str(tmp_path / "ref.fa"), "-d", str(out), "--no-stats", "--log-level", "DEBUG",
                 "--write-kept", str(tmp_path / "kept.bam")] + extra) == 0
    assert DEVICE in (out / "Runtime_log.txt").read_text()
    assert read_bam_file(tmp_path / "kept.bam") == (header, kept)


def test_a_file_the_device_path_gives_up_on_ends_the_run(tmp_path):
    """tests/golden/foreign.bam holds a record whose CIGAR lives in a CG tag: the device path hands such a file to the host
    decoder, and a run with --write-kept has no route through that one — the reason, then the error, exit code 1, no file."""
    from mapdamage_amd.main import main
    from tests.test_foreign_bam import reference, truth
    fasta.write_fasta(tmp_path / "ref.fa", reference(truth("full")[1]))
    out = tmp_path / "out"
    assert main(["-i", os.path.join(GOLDEN, "foreign.bam"), "-r", str(tmp_path / "ref.fa"), "-d", str(out), "--no-stats",
                 "--write-kept", str(tmp_path / "kept.bam")]) == 1
    log = (out / "Runtime_log.txt").read_text()
    assert "GPU decode path gave up" in log and "CG tag" in log
    assert "--write-kept is written by the device decode path" in log.split("GPU decode path gave up")[1]
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["ref.fa", "ref.fa.fai"]
    assert not any((out / f).exists() for f in FILES + ("write_kept.tsv",))


# ---------------------------------------------------------------------- 8. refusals at run time
def test_refusals_at_run_time(lib_data, tmp_path):
    b, ref = lib_data["batch"].slice(0, 200), lib_data["ref"]
    sam.write_sam(str(tmp_path / "in.sam"), b, ref.names, ref.lengths, RGS, [RGS[int(i)]["ID"] for i in b.lib])
    out = run(lib_data, tmp_path / "sam", tmp_path / "in.sam", "--write-kept", tmp_path / "kept.bam", rc=1)
    assert "--write-kept needs BAM input" in (out / "Runtime_log.txt").read_text()
    out = run(lib_data, tmp_path / "index", "in.bam", "--by-reference", "--write-kept", tmp_path / "kept.bam", "--write-groups", "1,5", rc=1)
    assert "--write-groups: group index 5 is outside 0..4" in (out / "Runtime_log.txt").read_text()
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["in.sam"]
    for folder in (tmp_path / "sam", tmp_path / "index"):
        assert not any((folder / f).exists() for f in FILES + ("write_kept.tsv",))
