"""A bgzip-compressed reference FASTA (BGZF under any name) through the library's loader: `pysam.FastaFile(options.ref)` of
mapdamage/main.py:115 reads `ref.fa.gz` with `.fai` + `.gzi` through htslib and builds missing indexes.  The compressed
blocks go to HBM, are inflated, CRC-checked and stripped of their line ends there (include/mdx.h mdx_set_reference_fasta);
`.fai` and `.gzi` of a file without them are built together (mdx_fasta_index).  `read_fasta` — Python's gzip — is the
second opinion."""

import gzip
import os
import pathlib
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from mapdamage_amd import fasta, sam
from mapdamage_amd.batch import Reference

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _upper_classes(seq: bytes) -> bytes:
    """ref.fetch(...).upper() with everything the loop does not tell apart folded: ACGT, '-', 'N' for the rest."""
    up = np.frombuffer(seq.upper(), np.uint8)
    out = np.full(up.shape, ord("N"), np.uint8)
    for ch in b"ACGT-":
        out[up == ch] = ch
    return out.tobytes()


def _block(data, level=6, before=b"", behind=b"", crc=None, isize=None):
    """One BGZF block by hand (SAM specification 4.1): other extra subfields in front of or behind 'BC', stored payloads
    (level 0), and trailers that lie."""
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = comp.compress(data) + comp.flush()
    xlen = len(before) + 6 + len(behind)
    bsize = 12 + xlen + len(payload) + 8 - 1
    extra = before + b"BC" + struct.pack("<HH", 2, bsize) + behind
    return (b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<H", xlen) + extra + payload +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def _write_blocks(path, text, size=0xFF00, eof=True, empty_at=None, **how):
    """``text`` as BGZF blocks of ``size`` bytes -> [(compressed offset, inflated offset)] of every block's start, the
    end-of-file block's included."""
    starts, out, coff = [], bytearray(), 0
    pieces = [text[lo:lo + size] for lo in range(0, len(text), size)]
    uoff = 0
    for i, piece in enumerate(pieces):
        if i == empty_at:
            starts.append((len(out), uoff))
            out += _block(b"", **how)
        starts.append((len(out), uoff))
        out += _block(piece, **how)
        uoff += len(piece)
    if eof:
        starts.append((len(out), uoff))
        out += _block(b"")
    pathlib.Path(path).write_bytes(bytes(out))
    return starts


def _bgzip(src, dst):
    """``src`` compressed as bgzip would (0xFF00-byte blocks and the end-of-file block), by the project's own writer."""
    with sam.BgzfWriter(dst, threads=2) as out:
        out.write(pathlib.Path(src).read_bytes())


def _gzi(starts):
    body = b"".join(struct.pack("<QQ", c, u) for c, u in starts)
    return struct.pack("<Q", len(starts)) + body


def _read_gzi(path):
    data = pathlib.Path(path).read_bytes()
    n, = struct.unpack_from("<Q", data)
    assert len(data) == 8 + 16 * n
    return [struct.unpack_from("<QQ", data, 8 + 16 * i) for i in range(n)]


SMALL = Reference(["a", "b", "empty", "c", "one"],
                  [b"ACGTTGCA" * 300 + b"AC", b"acgtnNRY-" * 211, b"", b"N" * 500 + b"GATTACA" * 150 + b"N" * 333, b"T"])


# ------------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("name", ["ref.fa.gz", "ref.fa.bgz"])
def test_a_bgzf_fasta_stays_on_disk_under_any_name(tmp_path, name):
    """By sniff, not by suffix.  (The parent commit read `*.gz` line by line in Python and took `*.bgz` for plain text.)"""
    fasta.write_fasta(tmp_path / "ref.fa", SMALL)
    _bgzip(tmp_path / "ref.fa", tmp_path / name)
    assert fasta.is_bgzf(tmp_path / name) and not fasta.is_bgzf(tmp_path / "ref.fa")
    got = fasta.reference_for_bam(tmp_path / name, ["c", "a"])
    assert isinstance(got, fasta.FastaOnDisk)
    assert got.path == str(tmp_path / name) and got.names == ["c", "a"] and got.lengths == [len(SMALL.seqs[3]), len(SMALL.seqs[0])]
    with pytest.raises(KeyError):
        fasta.reference_for_bam(tmp_path / name, ["absent"])


def test_a_plain_gzip_fasta_is_still_read_on_the_host(tmp_path, caplog):
    fasta.write_fasta(tmp_path / "ref.fa", SMALL)
    with gzip.open(tmp_path / "ref.fa.gz", "wb") as out:
        out.write((tmp_path / "ref.fa").read_bytes())
    assert not fasta.is_bgzf(tmp_path / "ref.fa.gz") and fasta.is_plain_gzip(tmp_path / "ref.fa.gz")
    names, seqs = fasta.read_fasta(tmp_path / "ref.fa.gz")
    with caplog.at_level("INFO"):
        got = fasta.reference_for_bam(tmp_path / "ref.fa.gz", ["c", "a", "one"])
    assert isinstance(got, Reference)
    by_name = dict(zip(names, seqs))
    assert got.names == ["c", "a", "one"] and got.seqs == [by_name[n] for n in got.names]
    assert "bgzip" in caplog.text and "plain gzip" in caplog.text


def test_fai_and_gzi_of_a_bgzf_fasta_are_built_together(tmp_path):
    # (sequences of a line at least: write_fasta's index gives the file's width to a shorter one, faidx its own length)
    ref = Reference(SMALL.names[:2] + ["c", "e"], SMALL.seqs[:2] + [SMALL.seqs[3], b"A" * 60])
    for width in (7, 60):
        plain, packed = tmp_path / ("w%d.fa" % width), tmp_path / ("w%d.fa.gz" % width)
        fasta.write_fasta(plain, ref, width=width)
        starts = _write_blocks(packed, plain.read_bytes(), size=1000)
        fasta.ensure_fasta_index(packed)
        # the .fai holds offsets into the inflated text: the uncompressed twin's, byte for byte
        assert pathlib.Path(str(packed) + ".fai").read_bytes() == pathlib.Path(str(plain) + ".fai").read_bytes()
        # bgzip's .gzi: every block behind the first, without the end-of-file block
        assert _read_gzi(str(packed) + ".gzi") == starts[1:-1]
        assert not [p for p in os.listdir(tmp_path) if p.endswith(".tmp")]
    # a .gzi that exists is left alone; a .fai alone gets its .gzi (htslib refuses the one without the other)
    packed = tmp_path / "w60.fa.gz"
    os.remove(str(packed) + ".fai")
    pathlib.Path(str(packed) + ".gzi").write_bytes(b"kept")
    fasta.ensure_fasta_index(packed)
    assert pathlib.Path(str(packed) + ".gzi").read_bytes() == b"kept"
    assert pathlib.Path(str(packed) + ".fai").read_bytes() == (tmp_path / "w60.fa.fai").read_bytes()
    os.remove(str(packed) + ".gzi")
    fasta.ensure_fasta_index(packed)
    assert _read_gzi(str(packed) + ".gzi") == starts[1:-1]
    # CR LF, a description behind the name and an empty last sequence, as uncompressed
    _write_blocks(tmp_path / "u.fa.bgz", b">x desc\r\nACGT\r\nAC\r\n>y\r\nGG\r\n>z\n", size=5)
    fasta.ensure_fasta_index(tmp_path / "u.fa.bgz")
    assert (tmp_path / "u.fa.bgz.fai").read_text() == "x\t6\t9\t4\t6\ny\t2\t23\t2\t4\nz\t0\t30\t0\t0\n"


def test_a_bgzf_fasta_that_cannot_be_indexed_leaves_nothing_behind(tmp_path):
    for name, text, message in (("v.fa.gz", b">x\nACGT\nAC\nACGT\n", "different line length"), ("w.fa.gz", b"ACGT\n", "not a FASTA")):
        _write_blocks(tmp_path / name, text, size=6)
        with pytest.raises(ValueError, match=message):
            fasta.ensure_fasta_index(tmp_path / name)
        assert set(os.listdir(tmp_path)) <= {"v.fa.gz", "w.fa.gz"}
    # a block whose trailer lies is an error of the index pass too, by its offset in the file
    text = b">x\n" + b"ACGT" * 100 + b"\n"
    starts = _write_blocks(tmp_path / "c.fa.gz", text, size=100)
    data = bytearray((tmp_path / "c.fa.gz").read_bytes())
    data[starts[3][0] - 8] ^= 0x55           # CRC32 of block 2
    (tmp_path / "c.fa.gz").write_bytes(bytes(data))
    with pytest.raises(ValueError, match="offset %d " % starts[2][0]):
        fasta.ensure_fasta_index(tmp_path / "c.fa.gz")
    assert not (tmp_path / "c.fa.gz.fai").exists() and not (tmp_path / "c.fa.gz.gzi").exists()
    # a second gzip member without the BC subfield: not a BGZF file
    (tmp_path / "m.fa.gz").write_bytes(_block(b">x\nAC\n") + gzip.compress(b"GT\n"))
    with pytest.raises(ValueError, match="BGZF"):
        fasta.ensure_fasta_index(tmp_path / "m.fa.gz")


# ------------------------------------------------------------------------------------------------------------------ GPU

def _loaded(eng, path, order, by_name):
    on_disk = fasta.reference_for_bam(path, order, missing_ok=True)
    assert isinstance(on_disk, fasta.FastaOnDisk)
    eng.set_reference(on_disk)
    assert on_disk.lengths == [len(by_name.get(n, b"")) for n in order]
    for tid, name in enumerate(order):
        seq = by_name.get(name, b"")
        assert eng.reference_fetch(tid, 0, len(seq)) == _upper_classes(seq), name


@pytest.mark.gpu
@pytest.mark.parametrize("gzi", [True, False])
@pytest.mark.parametrize("width,crlf,piece", [(60, False, 0), (7, False, 4096), (61, True, 4096), (1000, False, 65536)])
def test_bgzf_fasta_file_becomes_the_resident_reference(tmp_path, monkeypatch, width, crlf, piece, gzi):
    """The matrix of test_fasta_file_becomes_the_resident_reference on bgzipped twins, with and without the .gzi."""
    from mapdamage_amd import synth
    from mapdamage_amd.engine import DamageEngine, MdxError
    ref, _ = synth.config1_batch()
    extra = Reference(ref.names + ["odd", "tiny", "none"],
                      ref.seqs + [b"acgtRYKMnN-*xACGT" * 37 + b"A", b"T", b""])
    plain, path = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, extra, width=width)
    if crlf:
        plain.write_bytes(plain.read_bytes().replace(b"\n", b"\r\n"))
        os.remove(str(plain) + ".fai")
    # (the genome is a few kilobytes — one block of bgzip's: with a piece size, blocks small enough that a piece holds several
    # and the file several pieces)
    if piece:
        _write_blocks(path, plain.read_bytes(), size=997)
    else:
        _bgzip(plain, path)
    fasta.ensure_fasta_index(path)              # .fai and .gzi of the compressed file, built by the library
    os.remove(str(plain) + ".fai") if not crlf else None
    fasta.ensure_fasta_index(plain)             # ... and the uncompressed twin's: the same offsets, into the inflated text
    assert pathlib.Path(str(path) + ".fai").read_bytes() == pathlib.Path(str(plain) + ".fai").read_bytes()
    if not gzi:
        os.remove(str(path) + ".gzi")
        monkeypatch.setattr(fasta, "ensure_fasta_index", lambda p: None)      # (the loader walks the block headers instead)
    if piece:
        monkeypatch.setenv("MDX_FASTA_PIECE_BYTES", str(piece))
    order = ["tiny", ref.names[1], "absent", "odd", ref.names[0], ref.names[2], "none"]
    by_name = dict(zip(extra.names, extra.seqs))
    with DamageEngine([("*", "*")], 70, 10, 0) as eng:
        with pytest.raises(KeyError):
            fasta.reference_for_bam(path, order)
        _loaded(eng, path, order, by_name)
        stats = eng.fasta_load_stats()
        assert stats["inflated"] > 0 and stats["slabs"] >= (2 if piece == 4096 else 1)
        assert os.path.exists(str(path) + ".gzi") == gzi
        n1 = len(by_name[ref.names[1]])
        assert eng.reference_fetch(1, n1 - 5, n1) == _upper_classes(by_name[ref.names[1]][-5:])
        strict = fasta.FastaOnDisk(path, ["absent"], [0], missing_ok=False)
        with pytest.raises(MdxError, match="not found"):
            eng.set_reference(strict)


LAYOUTS = {
    "full_blocks": dict(size=0xFF00),
    "tiny_blocks": dict(size=23),                 # a 60-base line lies in three or four blocks
    "stored": dict(size=4000, level=0),
    "empty_in_the_middle": dict(size=3000, empty_at=2),
    "subfield_in_front": dict(size=3000, before=b"XY\x03\x00abc"),
    "subfield_behind": dict(size=3000, behind=b"ZZ\x01\x00q"),
    "no_eof_block": dict(size=3000, eof=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("gzi", ["none", "built", "with_eof_entry"])
def test_every_block_layout_loads_to_the_same_reference(tmp_path, layout, gzi):
    from mapdamage_amd.engine import DamageEngine
    big = Reference(SMALL.names + ["long"], SMALL.seqs + [(b"ACGTNacgtn" * 977 + b"GGC") * (30 if layout == "full_blocks" else 1)])
    plain, path = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, big, width=60)
    starts = _write_blocks(path, plain.read_bytes(), **LAYOUTS[layout])
    pathlib.Path(str(path) + ".fai").write_bytes(pathlib.Path(str(plain) + ".fai").read_bytes())
    if gzi == "built":
        fasta.ensure_fasta_index(path)
    elif gzi == "with_eof_entry":
        # (every block's start behind the first, the end-of-file block's too where the file has one)
        pathlib.Path(str(path) + ".gzi").write_bytes(_gzi(starts[1:]))
    order = ["long", "one", "c", "empty", "b", "a"]
    with DamageEngine([("*", "*")], 70, 10, 0) as eng:
        if gzi == "none":
            on_disk = fasta.FastaOnDisk(path, order, [0] * len(order))
            eng.set_reference(on_disk)
            assert not os.path.exists(str(path) + ".gzi")
            for tid, name in enumerate(order):
                seq = dict(zip(big.names, big.seqs))[name]
                assert eng.reference_fetch(tid, 0, len(seq)) == _upper_classes(seq), name
        else:
            _loaded(eng, path, order, dict(zip(big.names, big.seqs)))
        stats = eng.fasta_load_stats()
        assert stats["blocks"] == len(starts)
        # the reader's answer on the same file
        names, seqs = fasta.read_fasta(path)
        assert names == big.names and seqs == big.seqs


@pytest.mark.gpu
def test_a_stale_gzi_is_dropped_for_the_block_headers(tmp_path):
    from mapdamage_amd.engine import DamageEngine
    plain, path = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, SMALL, width=60)
    starts = _write_blocks(path, plain.read_bytes(), size=700)
    pathlib.Path(str(path) + ".fai").write_bytes(pathlib.Path(str(plain) + ".fai").read_bytes())
    pathlib.Path(str(path) + ".gzi").write_bytes(_gzi([(c + 3, u) for c, u in starts[1:-1]]))
    with DamageEngine([("*", "*")], 70, 10, 0) as eng:
        _loaded(eng, path, ["one", "a", "b", "c"], dict(zip(SMALL.names, SMALL.seqs)))


@pytest.mark.gpu
@pytest.mark.parametrize("gzi", [True, False])
def test_only_the_blocks_of_wanted_sequences_are_inflated(tmp_path, gzi):
    """A BAM that names one contig of a large FASTA must not inflate the genome."""
    from mapdamage_amd.engine import DamageEngine
    rng = np.random.default_rng(5)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 30_000)) for _ in range(8)] + [b"GATTACA" * 100]
    many = Reference(["s%d" % i for i in range(8)] + ["last"], seqs)
    plain, path = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, many, width=60)
    starts = _write_blocks(path, plain.read_bytes(), size=2000)
    pathlib.Path(str(path) + ".fai").write_bytes(pathlib.Path(str(plain) + ".fai").read_bytes())
    if gzi:
        fasta.ensure_fasta_index(path)
    n_blocks = len(starts)
    assert n_blocks > 120
    with DamageEngine([("*", "*")], 70, 10, 0) as eng:
        eng.set_reference(fasta.FastaOnDisk(path, ["last"], [0]))
        assert eng.reference_fetch(0, 0, 700) == b"GATTACA" * 100
        stats = eng.fasta_load_stats()
        # 700 bases and their line ends: 712 bytes of text lie in one or two blocks of 2000
        assert stats["blocks"] == n_blocks and 1 <= stats["inflated"] <= 2 and stats["slabs"] == 1
        assert stats["bytes"] < 2 * 2100
        eng.set_reference(fasta.FastaOnDisk(path, many.names, [0] * 9))
        stats = eng.fasta_load_stats()
        assert stats["inflated"] >= n_blocks - 2       # (a block that holds nothing but a header line's bytes, and the last one)
        for tid, seq in enumerate(seqs):
            assert eng.reference_fetch(tid, 0, len(seq)) == seq


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["payload", "crc", "isize"])
@pytest.mark.parametrize("gzi", [True, False])
def test_a_damaged_block_is_an_error_that_names_its_offset(tmp_path, damage, gzi):
    """Bad data, as tests/test_gpu_decode.py feeds the same inflater: a return code of the kernel, not a fault."""
    from mapdamage_amd.engine import DamageEngine, MdxError
    plain, path = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, SMALL, width=60)
    starts = _write_blocks(path, plain.read_bytes(), size=900)
    pathlib.Path(str(path) + ".fai").write_bytes(pathlib.Path(str(plain) + ".fai").read_bytes())
    if gzi:
        fasta.ensure_fasta_index(path)
    data = bytearray(path.read_bytes())
    hit = 3
    end = starts[hit + 1][0]
    if damage == "payload":
        data[(starts[hit][0] + 18 + end - 8) // 2] ^= 0xFF          # the middle of the payload (header 18 bytes, trailer 8)
    elif damage == "crc":
        data[end - 8] ^= 0x01
    else:
        data[end - 4:end] = struct.pack("<I", 901)
    path.write_bytes(bytes(data))
    with DamageEngine([("*", "*")], 70, 10, 0) as eng:
        with pytest.raises(MdxError, match="offset %d " % starts[hit][0]):
            eng.set_reference(fasta.FastaOnDisk(path, SMALL.names, [0] * len(SMALL.names)))
        # sequence 'one' lies in the last block: the damaged one is not read for it.  (Without a .gzi the inflated offsets are the
        # sums of the ISIZE fields in front: a wrong ISIZE then misplaces every block behind it, and only inflating the block
        # tells — htslib does not seek in such a file at all.)
        if gzi or damage != "isize":
            eng.set_reference(fasta.FastaOnDisk(path, ["one"], [0]))
            assert eng.reference_fetch(0, 0, 1) == b"T"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config1_L70_A10_Q0", "edge_L70_A10_Q0", "config1_L70_A10_Q20", "edge_L200_A25_Q10"])
def test_tables_over_the_loaded_bgzf_fasta_equal_the_reference_golden(tmp_path, name):
    from mapdamage_amd.engine import DamageEngine
    from util import Golden
    g = Golden(name)
    fasta.write_fasta(tmp_path / "ref.fa", g.ref, width=50)
    _bgzip(tmp_path / "ref.fa", tmp_path / "ref.fa.gz")
    with DamageEngine(g.libraries, g.length, g.around, g.minqual) as eng:
        eng.set_reference(fasta.reference_for_bam(tmp_path / "ref.fa.gz", g.ref.names))
        assert eng.fasta_load_stats()["inflated"] > 0
        eng.tabulate(g.batch, packed=True)
        g.check(eng.finish())


def _cli(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    out = subprocess.run([sys.executable, "-m", "mapdamage_amd"] + [str(a) for a in args], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    return out


@pytest.mark.gpu
def test_the_command_line_takes_a_bgzipped_reference(tmp_path):
    from util import Golden
    golden = "config1_L70_A10_Q0"
    g = Golden(golden)
    rgs = [{"ID": "rg%d" % i, "SM": s, "LB": l} for i, (s, l) in enumerate(g.meta["libraries"])]
    raw_lib = np.load(str(pathlib.Path(__file__).parent / "golden" / (golden + ".npz")))["lib"]
    bam = tmp_path / "in.bam"
    sam.write_bam(bam, g.batch, g.ref.names, g.ref.lengths, rgs, ["rg%d" % int(l) for l in raw_lib])
    plain, packed = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    fasta.write_fasta(plain, g.ref)
    _bgzip(plain, packed)
    fasta.ensure_fasta_index(packed)
    indexes = [pathlib.Path(str(packed) + ".fai"), pathlib.Path(str(packed) + ".gzi")]
    for run in ("indexed", "bare"):
        if run == "bare":
            for p in indexes:
                os.remove(p)
        out = tmp_path / run
        _cli(["-i", bam, "-r", packed, "-d", out, "--no-stats"])
        for name in ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt"):
            assert (out / name).read_text() == g.txt[name], (run, name)
        assert all(p.exists() for p in indexes)
        log = (out / "Runtime_log.txt").read_text()
        assert "bgzip-compressed FASTA, loaded by the device" in log and "Python reader" not in log
    # a plain gzip file with a ready .fai: the old path, the same tables
    slow = tmp_path / "slow.fa.gz"
    with gzip.open(slow, "wb") as handle:
        handle.write(plain.read_bytes())
    pathlib.Path(str(slow) + ".fai").write_bytes(pathlib.Path(str(plain) + ".fai").read_bytes())
    out = tmp_path / "plain_gzip"
    _cli(["-i", bam, "-r", slow, "-d", out, "--no-stats"])
    for name in ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt"):
        assert (out / name).read_text() == g.txt[name], name
    log = (out / "Runtime_log.txt").read_text()
    assert "Python reader" in log and "bgzip" in log and "loaded by the device" not in log
    assert not os.path.exists(str(slow) + ".gzi")
    # a reference that cannot be indexed: an error in the log and exit code 1, no traceback
    bad = tmp_path / "bad.fa.gz"
    _write_blocks(bad, b">x\nACGT\nAC\nACGT\n", size=6)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    res = subprocess.run([sys.executable, "-m", "mapdamage_amd", "-i", str(bam), "-r", str(bad), "-d", str(tmp_path / "bad"), "--no-stats"],
                         cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "Traceback" not in res.stderr
    assert "different line length" in (tmp_path / "bad" / "Runtime_log.txt").read_text()
