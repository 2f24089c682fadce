"""--write-index without a GPU: the yardstick (tests/bai_util.py) pinned on a file whose index is written out by hand and checked
against a scan of all records; the rule of mapdamage_amd/csrc/mdx_kept_index.h compiled for the host, as a library and as a
program under the sanitizers, against the yardstick's reg2bin and extent; mapdamage_amd/bai.py fed runs and member tables made
here against the yardstick's bytes for the file they describe; the command line's argument errors.

The builders below (``record``, ``raw_header``, ``write_members``, ``write_slabs``) also make the files of
tests/test_gpu_write_index.py."""

import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import bai_util as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mapdamage_amd", "csrc")
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MEMBER = 0xFF00
OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}


# ---------------------------------------------------------------------- builders
POOL = bytes(33 + b % 90 for b in np.random.default_rng(12).integers(0, 256, 1 << 16, dtype=np.uint8).tobytes())


def record(tid, pos, cigar=(), name=b"r", flag=0, size=None, mapq=30):
    """A BAM record with its block_size field: no bases, ``cigar`` = [(length, "M"), ...]; ``size``: its bytes in all, reached
    with a ZZ:Z tag of characters that do not compress away."""
    words = b"".join(struct.pack("<I", n << 4 | OPS[op]) for n, op in cigar)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, 0, -1, -1, 0) + name + b"\0" + words
    if size is not None:
        pad = size - 4 - len(body)
        assert pad == 0 or pad >= 4, (size, len(body))
        if pad:
            at = (pos * 31 + len(name) * 977) % (len(POOL) - pad)
            body += b"ZZZ" + POOL[at:at + pad - 4] + b"\0"
    return struct.pack("<i", len(body)) + body


def raw_header(refs, so="coordinate"):
    text = "@HD\tVN:1.6\tSO:%s\n" % so + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@RG\tID:rgA\tSM:s\tLB:l\n"
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out


def member(chunk, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(chunk) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body
            + struct.pack("<II", zlib.crc32(chunk), len(chunk)))


def write_members(path, chunks, level=6):
    """One BGZF member per chunk, then the marker; returns the members' file offsets (the marker's last)."""
    offsets, at = [], 0
    with open(path, "wb") as out:
        for chunk in chunks:
            offsets.append(at)
            at += out.write(member(chunk, level))
        offsets.append(at)
        out.write(EOF_MARKER)
    return offsets


def write_slabs(path, header, slabs):
    """The layout of --write-kept: the header in members of its own, every slab's stream (bytes) cut into members of 0xFF00,
    the last one as short as it comes."""
    chunks = []
    for piece in [header] + [s for s in slabs if s]:
        chunks += [piece[lo:lo + MEMBER] for lo in range(0, len(piece), MEMBER)]
    return write_members(path, chunks)


def write_sorted_input(path, refs, records, block_bytes=None, level=6):
    """An input file: header and records back to back in blocks of ``block_bytes`` (None: 0xFF00) whatever the borders
    (``level`` 0: stored, so that the blocks' sizes do not depend on what the records hold)."""
    data = raw_header(refs) + b"".join(records)
    step = block_bytes or MEMBER
    write_members(path, [data[lo:lo + step] for lo in range(0, len(data), step)], level)


# ---------------------------------------------------------------------- 1. the yardstick, by hand
REFS3 = [("chrA", 100_000), ("chrB", 50_000), ("chrC", 40_000)]


def test_yardstick_on_a_file_indexed_by_hand(tmp_path):
    recs = [record(0, 100, [(50, "M")], b"r0"),                          # window 0, bin 4681
            record(0, 200, [(50, "M")], b"r1"),                          # the same bin: one chunk with r0
            record(0, 16_000, [(1000, "M")], b"r2"),                     # crosses 16384: level 2^17, bin 585; windows 0 and 1
            record(0, 40_000, [(10, "=")], b"r3"),                       # window 2, bin 4683
            record(2, 0, [], b"r4"),                                     # no operations: one base; bin 4681
            record(2, 33_000, [(10, "M"), (50, "N"), (40, "M")], b"r5")]  # 33000..33100: window 2, bin 4683
    sizes = [len(r) for r in recs]
    assert sizes == [43, 43, 43, 43, 39, 51]
    header = raw_header(REFS3)
    stream = b"".join(recs)
    # members: the header; r0, r1 and ten bytes of r2; the rest of r2, r3, r4; r5
    cut1, cut2 = 43 + 43 + 10, 4 * 43 + 39
    at = write_members(tmp_path / "hand.bam", [header, stream[:cut1], stream[cut1:cut2], stream[cut2:]])
    m1, m2, m3, eof = at[1], at[2], at[3], at[4]
    assert 0 < m1 < m2 < m3 < eof < 1 << 16
    bam = Y.Bam(tmp_path / "hand.bam")
    assert [(r["tid"], r["pos"], r["end"]) for r in bam.records] == [(0, 100, 150), (0, 200, 250), (0, 16_000, 17_000), (0, 40_000, 40_010),
                                                                     (2, 0, 1), (2, 33_000, 33_100)]
    v = lambda m, u: m << 16 | u      # noqa: E731
    r0, r1_end, r2, r2_end = v(m1, 0), v(m1, 86), v(m1, 86), v(m2, 33)
    r3, r3_end, r4 = v(m2, 33), v(m2, 76), v(m2, 76)
    r4_end = r5 = v(m3, 0)          # r4 ends where its member does: the next member's first byte
    r5_end = v(eof, 0)              # ... and r5 at the end of the last one: the marker
    want = b"BAI\x01" + struct.pack("<i", 3)
    want += struct.pack("<i", 4)
    want += struct.pack("<IiQQ", 585, 1, r2, r2_end)
    want += struct.pack("<IiQQ", 4681, 1, r0, r1_end)
    want += struct.pack("<IiQQ", 4683, 1, r3, r3_end)
    want += struct.pack("<IiQQQQ", 37450, 2, r0, r3_end, 4, 0)
    want += struct.pack("<iQQQ", 3, r0, r2, r3)
    want += struct.pack("<ii", 0, 0)
    want += struct.pack("<i", 3)
    want += struct.pack("<IiQQ", 4681, 1, r4, r4_end)
    want += struct.pack("<IiQQ", 4683, 1, r5, r5_end)
    want += struct.pack("<IiQQQQ", 37450, 2, r4, r5_end, 2, 0)
    want += struct.pack("<iQQQ", 3, r4, r5, r5)         # window 1 is untouched: the value of window 2
    want += struct.pack("<Q", 0)
    got = Y.build_index(bam)
    assert got == want
    parsed = Y.parse_index(got)
    assert parsed[0][0][4681] == [(r0, r1_end)] and parsed[1] == ({}, []) and parsed[2][1] == [r4, r5, r5]
    # ... and the reader finds through it what a scan finds
    for tid, beg, end, names in [(0, 0, 100, []), (0, 0, 101, ["r0"]), (0, 149, 201, ["r0", "r1"]), (0, 16_383, 16_385, ["r2"]),
                                 (0, 16_999, 40_000, ["r2"]), (0, 17_000, 40_000, []), (0, 0, 100_000, ["r0", "r1", "r2", "r3"]),
                                 (1, 0, 50_000, []), (2, 0, 1, ["r4"]), (2, 1, 33_000, []), (2, 33_020, 33_030, ["r5"]), (2, 33_100, 40_000, [])]:
        found = Y.query(bam, parsed, tid, beg, end)
        assert found == Y.brute(bam, tid, beg, end), (tid, beg, end)
        assert [Y.Bam.record_at(bam, bam.stream.index(f))["name"] for f in found] == names, (tid, beg, end)


# ---------------------------------------------------------------------- 2. query against a scan
def sorted_records(rng, refs, n, max_span=3000, size_range=(60, 400)):
    """n records in coordinate order over ``refs``: spans of every size up to max_span, some without operations, some with an N."""
    tids = np.sort(rng.integers(0, len(refs), n))
    out = []
    for tid in range(len(refs)):
        k = int((tids == tid).sum())
        for i, pos in enumerate(np.sort(rng.integers(0, refs[tid][1] - max_span - 1, k))):
            kind = rng.integers(0, 10)
            span = int(rng.integers(1, max_span))
            cigar = [] if kind == 0 else [(span // 3 + 1, "M"), (span // 3, "N"), (span // 3 + 1, "M")] if kind == 1 else \
                [(3, "S"), (span, "M"), (2, "I")] if kind == 2 else [(span, "M")]
            size = int(rng.integers(*size_range)) + 4 * len(cigar)
            out.append(record(tid, int(pos), cigar, b"q%d_%d" % (tid, i), size=size))
    return out


def test_query_equals_a_scan_on_a_sorted_file(tmp_path):
    rng = np.random.default_rng(5)
    refs = [("one", 3_000_000), ("none", 1000), ("two", 200_000)]
    recs = sorted_records(rng, [refs[0], ("skip", 4000), refs[2]], 4000)
    recs = [r for r in recs if struct.unpack_from("<i", r, 4)[0] != 1]          # the middle reference stays empty
    write_sorted_input(tmp_path / "in.bam", refs, recs, block_bytes=5000)
    bam = Y.Bam(tmp_path / "in.bam")
    assert len(bam.records) == len(recs) > 2500
    index = Y.parse_index(Y.build_index(bam))
    assert index[1] == ({}, []) and len(index[0][1]) > 100 and len(index[0][0]) > 100
    n_found = 0
    for _ in range(60):
        tid = int(rng.integers(0, 3))
        beg = int(rng.integers(0, refs[tid][1]))
        end = min(refs[tid][1], beg + int(rng.choice([1, 10, 1000, 20_000, 500_000])))
        found = Y.query(bam, index, tid, beg, end)
        assert found == Y.brute(bam, tid, beg, end), (tid, beg, end)
        n_found += len(found)
    assert n_found > 1000
    assert Y.query(bam, index, 0, 0, 3_000_000) == [r["bytes"] for r in bam.records if r["tid"] == 0]


# ---------------------------------------------------------------------- 3. the rule, compiled for the host
def rule_cases():
    """(pos, cigar words, sequence length): starts and ends on, before and behind every multiple-of-a-level border, zero-span
    CIGARs, N operations, extents that leave the sequence or BAI's 2^29."""
    cases = []
    top = 1 << 29
    for shift in (14, 17, 20, 23, 26):
        step = 1 << shift
        for k in sorted({1, 2, 3, 7, (top >> shift) - 1, (top >> shift) // 2}):
            border = k * step
            for d_pos in (-2, -1, 0, 1):
                for d_end in (-1, 0, 1, 2):
                    for span in (1, 2, 100, step - 1, step, step + 1):
                        # an extent that ends at border + d_end, and one that starts at border + d_pos
                        for pos in (border + d_end - span, border + d_pos):
                            if 0 <= pos and pos + span <= top:
                                cases.append((pos, [span << 4 | 0], top))
    for pos in (0, 5, 16_383, 16_384, top - 1):
        for cigar in ([], [7 << 4 | OPS["S"]], [7 << 4 | OPS["I"], 3 << 4 | OPS["H"], 1 << 4 | OPS["P"]], [0 << 4 | OPS["M"]]):
            cases.append((pos, cigar, top))                                     # nothing consumed: one base
    for pos in (10, 16_000, (1 << 26) - 50):
        cases.append((pos, [30 << 4 | OPS["M"], 100_000 << 4 | OPS["N"], 20 << 4 | OPS["M"]], top))
        cases.append((pos, [5 << 4 | OPS["="], 2 << 4 | OPS["X"], 9 << 4 | OPS["D"], 4 << 4 | OPS["I"], 1 << 4 | OPS["N"]], top))
        cases.append((pos, [(1 << 27) << 4 | OPS["N"], 1 << 4 | OPS["M"]], top))
    # not placeable: behind the sequence's end, behind 2^29, a negative position
    cases += [(990, [11 << 4], 1000), (990, [10 << 4], 1000), (top - 10, [11 << 4], 1 << 30), (top - 10, [10 << 4], 1 << 30),
              (-1, [5 << 4], top), (0, [0xFFFFFFF << 4 | OPS["N"]] * 3, 1 << 31), (999, [], 1000), (1000, [], 1000)]
    return cases


def expected(pos, cigar, length):
    end = Y.extent_end(pos, cigar)
    placeable = pos >= 0 and end <= length and end <= 1 << 29
    return end, Y.reg2bin(pos, end) if placeable else 0xFFFFFFFF


@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("index") / "kept_index_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "kept_index_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.kept_index_windows_host.restype = ctypes.c_uint64
    lib.kept_index_windows_host.argtypes = [ctypes.c_int64]
    lib.kept_index_placeable_host.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    lib.kept_index_in_order_host.argtypes = [ctypes.c_int32] * 4
    return lib


def test_rule_against_the_yardstick(host_rule):
    cases = rule_cases()
    assert len(cases) > 2000
    by_length = {}
    for case in cases:
        by_length.setdefault(case[2], []).append(case)
    levels = set()
    for length, group in by_length.items():
        pos = np.asarray([c[0] for c in group], np.int32)
        off = np.concatenate([[0], np.cumsum([len(c[1]) for c in group])]).astype(np.uint32)
        words = np.asarray([w for c in group for w in c[1]] + [0], np.uint32)
        end, bins = np.zeros(len(group), np.int64), np.zeros(len(group), np.uint32)
        host_rule.kept_index_host(ctypes.c_int64(len(group)), pos.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p),
                                  words.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(length), end.ctypes.data_as(ctypes.c_void_p),
                                  bins.ctypes.data_as(ctypes.c_void_p))
        want = [expected(*c) for c in group]
        assert end.tolist() == [w[0] for w in want]
        assert bins.tolist() == [w[1] for w in want]
        levels |= {sum(b >= o for o in (1, 9, 73, 585, 4681)) for b in bins.tolist() if b != 0xFFFFFFFF}
    assert levels == {0, 1, 2, 3, 4, 5}             # every level of the binning scheme came by
    assert expected(990, [11 << 4], 1000)[1] == 0xFFFFFFFF and expected(990, [10 << 4], 1000)[1] == 4681
    assert expected(999, [], 1000) == (1000, 4681) and expected(1000, [], 1000)[1] == 0xFFFFFFFF


def test_rule_placeable_order_windows(host_rule):
    lens = np.asarray([1000, 1 << 29, (1 << 29) + 5, 0], np.int64)
    p = lens.ctypes.data_as(ctypes.c_void_p)
    place = lambda tid, pos, end: bool(host_rule.kept_index_placeable_host(tid, pos, end, 4, p))       # noqa: E731
    assert place(0, 0, 1) and place(0, 999, 1000) and not place(0, 999, 1001) and not place(0, -1, 5)
    assert place(1, (1 << 29) - 1, 1 << 29) and not place(2, 1 << 29, (1 << 29) + 1) and not place(2, (1 << 29) - 1, (1 << 29) + 1)
    assert not place(-1, 0, 1) and not place(4, 0, 1) and not place(3, 0, 1)
    order = lambda a, b: bool(host_rule.kept_index_in_order_host(a[0], a[1], b[0], b[1]))             # noqa: E731
    assert order((0, 5), (0, 5)) and order((0, 5), (0, 6)) and not order((0, 6), (0, 5))
    assert order((0, 900), (1, 0)) and not order((1, 0), (0, 900)) and order((-1, -1), (0, 0))
    assert [host_rule.kept_index_windows_host(n) for n in (-4, 0, 1, 16_384, 16_385, 1 << 29)] == [0, 0, 1, 1, 2, 1 << 15]


def test_rule_under_the_sanitizers(tmp_path):
    exe = tmp_path / "kept_index"
    subprocess.check_call(["c++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DKEPT_INDEX_MAIN", "-I", CSRC,
                           os.path.join(ROOT, "tests", "kept_index_host.cpp"), "-o", str(exe)])
    cases = rule_cases()
    with open(tmp_path / "cases.bin", "wb") as out:
        for pos, cigar, length in cases:
            end, b = expected(pos, cigar, length)
            out.write(struct.pack("<iqIqI", pos, length, len(cigar), end, b) + struct.pack("<%dI" % len(cigar), *cigar))
    done = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, timeout=120)
    assert done.returncode == 0, done.stdout.decode()[-2000:] + done.stderr.decode()[-4000:]
    assert done.stdout.decode().splitlines()[-1] == "%d extents placed, 0 wrong" % len(cases) and not done.stderr


# ---------------------------------------------------------------------- 4. the assembler
def runs_of(records, stream_base):
    """What the device hands back for one slab, from the records themselves (bytes with block_size, in file order): the runs
    (bai.RUN_DTYPE) and {(tid, window): lowest stream offset}."""
    from mapdamage_amd.bai import RUN_DTYPE
    runs, linear, at = [], {}, stream_base
    for j, r in enumerate(records):
        size, tid, pos, l_name, _q, _b, n_cigar = struct.unpack_from("<iiiBBHH", r, 0)
        end = Y.extent_end(pos, struct.unpack_from("<%dI" % n_cigar, r, 36 + l_name))
        b = Y.reg2bin(pos, end)
        if runs and runs[-1][0] == tid and runs[-1][1] == b:
            runs[-1][3], runs[-1][5] = at + len(r), j + 1
        else:
            runs.append([tid, b, at, at + len(r), j, j + 1])
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            linear.setdefault((tid, w), at)
        at += len(r)
    return np.array([tuple(r) for r in runs], RUN_DTYPE), linear


def linear_array(lengths, minima):
    from mapdamage_amd.bai import linear_windows
    windows = linear_windows(lengths)
    first = np.concatenate([[0], np.cumsum(windows)])
    out = np.full(int(first[-1]), 0xFFFFFFFFFFFFFFFF, np.uint64)
    for (tid, w), at in minima.items():
        out[first[tid] + w] = min(int(out[first[tid] + w]), at)
    return out


def assemble(path, refs, slabs):
    """``slabs``: lists of records.  The file as --write-kept lays it out, and bai.py's index of it from runs and member sizes."""
    from mapdamage_amd.bai import BaiAssembler, member_sizes
    header = raw_header(refs)
    streams = [b"".join(s) for s in slabs]
    write_slabs(path, header, streams)
    data = open(path, "rb").read()
    asm = BaiAssembler([n for _, n in refs])
    file_at = int(member_sizes(member(header[:MEMBER])).sum()) if len(header) <= MEMBER else None
    assert file_at is not None
    base, minima = 0, {}
    for records, stream in zip(slabs, streams):
        if not records:
            continue
        runs, lin = runs_of(records, base)
        for key, at in lin.items():
            minima.setdefault(key, at)
        n_members = (len(stream) + MEMBER - 1) // MEMBER
        sizes, at = [], file_at
        for _ in range(n_members):
            sizes.append(struct.unpack_from("<H", data, at + 16)[0] + 1)
            at += sizes[-1]
        assert (member_sizes(data[file_at:at]) == sizes).all()
        asm.add_slab(base, file_at, sizes, len(stream), runs)
        base += len(stream)
        file_at = at
    assert data[file_at:] == EOF_MARKER
    return asm, asm.finish(linear_array([n for _, n in refs], minima))


def border_slabs():
    """Two slabs.  In the first one record ends exactly at stream offset 0xFF00, one straddles 2 * 0xFF00, and the slab ends on a
    member border; its last run goes on in the second slab, which ends inside a member."""
    refs = [("chr1", 1 << 29), ("empty", 5000), ("chr3", 300_000)]
    sizes = [1020] * 64 + [1000] * 66 + [1000] * 63 + [1560]
    assert sum(sizes[:64]) == MEMBER and sum(sizes[:129]) < 2 * MEMBER < sum(sizes[:130]) and sum(sizes) == 3 * MEMBER
    pos = 100_000
    first = []
    for i, size in enumerate(sizes):
        first.append(record(0, pos, [(100, "M")], b"a%d" % i, size=size))
        pos += 300 if i % 50 else 70_000            # every 50th record jumps over windows
    first_bin = Y.reg2bin(pos - 300, pos - 200)
    second = [record(0, pos + 10 * i, [(20, "M")], b"b%d" % i, size=500) for i in range(5)]
    assert Y.reg2bin(pos, pos + 20) == first_bin == Y.reg2bin(pos + 40, pos + 60)          # the run crosses the slab border
    second += [record(0, (1 << 29) - 200, [(200, "M")], b"top", size=300), record(2, 0, [], b"c0", size=100),
               record(2, 16_000, [(1000, "M"), (100_000, "N"), (10, "M")], b"c1", size=700)]
    assert sum(len(r) for r in second) % MEMBER
    return refs, [first, [], second]


def test_assembler_against_the_yardstick(tmp_path):
    refs, slabs = border_slabs()
    asm, got = assemble(tmp_path / "borders.bam", refs, slabs)
    bam = Y.Bam(tmp_path / "borders.bam")
    assert [r["bytes"] for r in bam.records] == slabs[0] + slabs[2]
    want = Y.build_index(bam)
    assert got == want
    parsed = Y.parse_index(got)
    assert asm.n_references == 2 and asm.n_chunks == sum(len(c) for bins, _ in parsed for b, c in bins.items() if b != 37450)
    # the end-of-member rule was needed: chunk ends and starts with uoffset 0 are there, the last end is the marker's offset
    members = {m[0] for m in bam.members}
    ends = [c[1] for bins, _ in parsed for cs in bins.values() for c in cs]
    assert any(e & 0xFFFF == 0 and e >> 16 in members for e in ends) and max(ends) == bam.members[-1][0] << 16
    # the run across the slab border is one chunk: it begins in the first slab's members and ends in the second's
    first_slab_end = bam.members[1 + 3][0]
    assert any(c[0] >> 16 < first_slab_end <= c[1] >> 16 and c[1] & 0xFFFF for bins, _ in parsed for b, cs in bins.items() if b != 37450 for c in cs)
    for tid, beg, end in [(0, 0, 1 << 29), (0, 100_000, 100_001), (0, 170_000, 171_000), (0, (1 << 29) - 1, 1 << 29), (1, 0, 5000),
                          (2, 0, 1), (2, 50_000, 60_000), (2, 117_005, 117_006), (2, 117_010, 300_000)]:
        assert Y.query(bam, parsed, tid, beg, end) == Y.brute(bam, tid, beg, end), (tid, beg, end)


def test_assembler_small_cases(tmp_path):
    from mapdamage_amd.bai import BaiAssembler, linear_windows, member_sizes
    refs = [("chr1", 100_000), ("chr2", 20_000)]
    # nothing written: a valid index without bins
    asm, got = assemble(tmp_path / "empty.bam", refs, [[], []])
    assert got == Y.build_index(Y.Bam(tmp_path / "empty.bam")) == b"BAI\x01" + struct.pack("<iiiiiQ", 2, 0, 0, 0, 0, 0)
    assert asm.n_references == 0 and asm.n_chunks == 0
    # one record; one record per slab, each a run of its own; the same bin in every slab: one chunk
    for name, slabs in [("one", [[record(1, 5, [(10, "M")])]]),
                        ("each", [[record(0, 5, [(10, "M")])], [record(0, 20_000, [(10, "M")])], [record(1, 0, [])]]),
                        ("joined", [[record(0, 5, [(10, "M")])], [record(0, 6, [(10, "M")])], [], [record(0, 7, [(10, "M")]), record(0, 70_000, [])]])]:
        asm, got = assemble(tmp_path / (name + ".bam"), refs, slabs)
        assert got == Y.build_index(Y.Bam(tmp_path / (name + ".bam"))), name
    assert asm.n_chunks == 2
    assert linear_windows([0, 1, 16_384, 16_385, -3]) == [0, 1, 1, 2, 0]
    with pytest.raises(ValueError, match="not a BGZF member"):
        member_sizes(b"\0" * 30)
    with pytest.raises(ValueError, match="cut short"):
        member_sizes(EOF_MARKER + EOF_MARKER[:20])
    with pytest.raises(ValueError, match="make 2 members"):
        BaiAssembler([1000]).add_slab(0, 100, [50], MEMBER + 1, runs_of([record(0, 5)], 0)[0])
    with pytest.raises(ValueError, match="does not begin where"):
        asm = BaiAssembler([1000])
        asm.add_slab(0, 100, [50], 40, runs_of([record(0, 5)], 0)[0])
        asm.add_slab(41, 150, [50], 40, runs_of([record(0, 6)], 41)[0])
    with pytest.raises(ValueError, match="words"):
        BaiAssembler([1000]).finish(np.zeros(3, np.uint64))


# ---------------------------------------------------------------------- 5. the command line
def error_of(tmp_path, capsys, *args):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit) as err:
        parse_args(["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out"), "--no-stats"] + [str(a) for a in args])
    assert err.value.code == 2
    return capsys.readouterr().err


def test_argument_errors(tmp_path, capsys):
    from mapdamage_amd.main import parse_args
    out = tmp_path / "kept.bam"
    base = ["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out"), "--no-stats"]
    assert "--write-index needs --write-kept" in error_of(tmp_path, capsys, "--write-index")
    assert "--write-index needs --write-kept" in error_of(tmp_path, capsys, "--write-index", "--by-pmd-score")
    # every restriction of --write-kept stands
    assert "not with --host-decode" in error_of(tmp_path, capsys, "--write-kept", out, "--write-index", "--host-decode")
    assert "cannot be combined with --gpus 2" in error_of(tmp_path, capsys, "--write-kept", out, "--write-index", "--gpus", "2")
    assert "cannot be combined with -n 1000" in error_of(tmp_path, capsys, "--write-kept", out, "--write-index", "-n", "1000")
    assert "its directory does not exist" in error_of(tmp_path, capsys, "--write-kept", tmp_path / "missing" / "k.bam", "--write-index")
    o = parse_args(base)
    assert o.write_index is False
    o = parse_args(base + ["--write-kept", str(out), "--write-index"])
    assert o.write_index is True and o.write_kept == out
    for extra in (["--by-pmd-score", "--write-groups", "1", "--tag-group", "XG", "--tag-pmd-score", "DS"], ["--regions", "p.bed", "--only-regions"],
                  ["--min-mapq", "25", "-n", "0.5"], ["-Q", "20", "--chunk-mb", "64"]):
        assert parse_args(base + ["--write-kept", str(out), "--write-index"] + extra).write_index


def test_a_sequence_bai_cannot_address_ends_the_run_at_the_header(tmp_path, monkeypatch):
    """A header sequence longer than 2^29: the error comes once the header is read — no reference file is opened (there is
    none), no record is read (there is none that could be: the file ends behind its header)."""
    from mapdamage_amd.main import main
    monkeypatch.setenv("MDX_NO_WARM", "1")
    refs = [("short", 1000), ("long", (1 << 29) + 1)]
    write_members(tmp_path / "in.bam", [raw_header(refs)])
    out = tmp_path / "out"
    assert main(["-i", str(tmp_path / "in.bam"), "-r", str(tmp_path / "none.fa"), "-d", str(out), "--no-stats",
                 "--write-kept", str(tmp_path / "kept.bam"), "--write-index"]) == 1
    log = (out / "Runtime_log.txt").read_text()
    assert "--write-index: reference sequence long has 536870913 bases" in log and "BAI cannot address" in log and "CSI" in log
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["in.bam"]
    # a sequence of exactly 2^29 bases passes the check (the run then ends on the missing reference file)
    write_members(tmp_path / "in.bam", [raw_header([("exact", 1 << 29)])])
    assert main(["-i", str(tmp_path / "in.bam"), "-r", str(tmp_path / "none.fa"), "-d", str(tmp_path / "out2"), "--no-stats",
                 "--write-kept", str(tmp_path / "kept.bam"), "--write-index"]) == 1
    assert "--write-index" not in (tmp_path / "out2" / "Runtime_log.txt").read_text().split("Started with the command")[1].split("\n", 1)[1]
