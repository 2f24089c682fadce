"""bgzip-compressed SAM text inflated, CRC-checked and parsed on the GPU (include/mdx.h mdx_gsam_*, BGZF input): the columns
equal sam.read_sam's whatever the block and slab sizes cut through, any BGZF layout is taken, mdx_gsam_tell_bgzf names the line
the next slab starts with, the command line writes the reference's tables from a file, a pipe and `< x.sam.gz` with no
fallback, damage and odd lines end where the host parser ends them, and plain gzip is the host's.  htslib reads compressed
SAM as SAM (its documentation; unpinned at the pysam boundary); the fixtures are the project's own BGZF writer's and blocks
made by hand."""
import gzip

import numpy as np
import pytest

from mapdamage_amd import fasta, sam
from tests.test_fasta_bgzf import _bgzip, _block, _write_blocks
from tests.test_gpu_distributed import _cli as _cli_ranks
from tests.test_gpu_pipe_input import FILES, GOLDENS, _cli, _main_on_pipe, _tables
from tests.test_gpu_sam_decode import (LIB_OF, _device_columns, _edge_lines, _genome, _golden_sam, _odd, _pack, _reads, _write_sam)

pytestmark = pytest.mark.gpu

LIBS = [("s1", "lib1"), ("s2", "lib2")]
DEVICE = "Decode path: device; fallbacks from the device path: 0"


def _long_line():
    """One read of 20 000 bases with qualities: longer than a 64 KiB block's worth of small blocks and than a 4 096-byte slab."""
    seq = "ACGTTGCAAC" * 2000
    qual = "".join(chr(33 + (5 * i) % 40) for i in range(20_000))
    return "long1\t0\tchr1\t1000\t30\t20000M\t*\t0\t0\t%s\t%s\tRG:Z:rg_b2" % (seq, qual)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The 3 000-record, two-library set of test_columns_equal_read_sam with its edge lines and the long read, without a
    final newline: (reference, the text's path, read_sam's columns)."""
    tmp = tmp_path_factory.mktemp("samgz")
    ref = _genome()
    b, rg = _reads(ref, 3000)
    path = tmp / "x.sam"
    _write_sam(path, ref, b, rg, extra=_edge_lines() + [_long_line()], newline_at_end=False)
    return ref, path, sam.read_sam(str(path))


def _check(cols, missing, host, minqual, packed):
    hb = host.batch
    want_lib = np.asarray([LIB_OF.get(r, 0xFFFF) if r is not None else 0xFFFF for r in host.rg], np.uint16)
    seq_lens = np.diff(hb.seq_off.astype(np.int64))
    got = {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in cols.items() if k not in ("qual", "seq")}
    assert got["flag"].shape[0] == hb.n
    if hb.n == 0:
        return
    np.testing.assert_array_equal(got["flag"] & 0x3FFF, hb.flag)
    for name in ("tid", "pos", "tlen", "cigar"):
        np.testing.assert_array_equal(got[name], getattr(hb, name), err_msg=name)
    np.testing.assert_array_equal(got["clen"], np.diff(hb.cigar_off))
    np.testing.assert_array_equal(got["slen"], seq_lens)
    np.testing.assert_array_equal(got["lib"], want_lib)
    first = hb.qual[np.minimum(hb.seq_off[:-1].astype(np.int64), hb.qual.shape[0] - 1)]
    has_qual = (seq_lens > 0) & (first != 0xFF)
    np.testing.assert_array_equal((got["flag"] & 0x4000) != 0, has_qual)
    if packed:
        want = _pack(hb.seq, hb.qual, hb.seq_off, minqual)
        want = np.stack([want & 15, want >> 4], 1).reshape(-1)[:hb.seq.shape[0]]
        np.testing.assert_array_equal(np.concatenate(cols["seq"]), want)
    else:
        np.testing.assert_array_equal(np.concatenate(cols["seq"]), hb.seq)
    if minqual == 0:
        np.testing.assert_array_equal(np.concatenate(cols["qual"]), hb.qual)
    else:
        qmin = np.asarray([hb.qual[a:z].min() if z > a else 0xFF for a, z in zip(hb.seq_off[:-1], hb.seq_off[1:])])
        np.testing.assert_array_equal((got["flag"] & 0x8000) != 0, qmin >= minqual)
        assert missing == bool(((hb.flag & 0xF04) == 0)[~has_qual].any())


@pytest.mark.parametrize("chunk", [1 << 28, 4096])
@pytest.mark.parametrize("block", [0xFF00, 301])
def test_columns_equal_read_sam(tmp_path, case, block, chunk):
    """At 301 bytes every line straddles blocks; at 4 096 compressed bytes lines straddle slabs, and the long line spans
    several of them (and outgrows the gap in front of a slab's text)."""
    from mapdamage_amd.engine import DamageEngine
    ref, path, host = case
    gz = tmp_path / "x.sam.gz"
    _write_blocks(gz, path.read_bytes(), size=block)
    for minqual, packed in ((0, False), (0, True), (20, True)):
        with DamageEngine(LIBS, 70, 10, minqual) as eng:
            eng.set_reference(ref)
            cols, missing = _device_columns(eng, gz, chunk, minqual, packed)
        _check(cols, missing, host, minqual, packed)


def _layouts(text):
    """name -> the BGZF bytes of ``text`` (or of part of it), by hand."""
    lines = text.split(b"\n")
    cuts = np.cumsum([len(x) + 1 for x in lines])
    a, b, c = int(cuts[len(lines) // 4]), int(cuts[len(lines) // 2]), int(cuts[3 * len(lines) // 4])
    head = b"".join(x + b"\n" for x in lines if x.startswith(b"@"))
    bl = lambda lo, hi, **how: b"".join(_block(text[i:min(hi, i + 5000)], **how) for i in range(lo, hi, 5000))
    return {
        "empty blocks first, in the middle and last": (text, _block(b"") + bl(0, b) + _block(b"") + _block(b"") + bl(b, len(text)) + _block(b"") + _block(b"")),
        "an end-of-file block in the middle and none at the end": (text, bl(0, a) + _block(b"") + bl(a, len(text))),
        "stored blocks": (text, bl(0, a) + bl(a, b, level=0) + bl(b, len(text)) + _block(b"")),
        "extra subfields around BC": (text, bl(0, len(text), before=b"XY\x03\x00abc", behind=b"ZZ\x00\x00") + _block(b"")),
        # (a: behind a '\n' — the first block ends exactly at it; the third begins with one)
        "a block that ends at a newline and one that begins with it": (text, _block(text[:a]) + _block(text[a:c - 1]) + _block(text[c - 1:]) + _block(b"")),
        "header only": (head, _block(head[:100]) + _block(head[100:]) + _block(b"")),
        "nothing but an end-of-file block": (b"", _block(b"")),
    }


@pytest.mark.parametrize("chunk", [1 << 28, 6000])
def test_layouts_by_hand(tmp_path, chunk):
    from mapdamage_amd.engine import DamageEngine
    ref = _genome()
    b, rg = _reads(ref, 300, seed=6)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg, extra=_edge_lines())
    with DamageEngine(LIBS, 70, 10, 0) as eng:
        eng.set_reference(ref)
        for k, (name, (text, data)) in enumerate(_layouts(path.read_bytes()).items()):
            plain, gz = tmp_path / ("t%d.sam" % k), tmp_path / ("t%d.sam.gz" % k)
            plain.write_bytes(text)
            gz.write_bytes(data)
            assert gzip.decompress(data) == text, name
            host = sam.read_sam(str(plain))
            cols, missing = _device_columns(eng, gz, chunk, 0, False)
            assert sum(len(x) for x in cols["flag"]) == host.batch.n, name
            _check(cols, missing, host, 0, False)
            if k >= 5:
                # zero records and at_end at the first call — and the sniff sends such a file here
                assert host.batch.n == 0 and not cols["flag"], name
                assert sam.input_format(str(gz)) == sam.SAM_BGZF, name
                with sam.GpuSamStream(eng, str(gz), readgroups=list(LIB_OF.items())) as g:
                    assert g.next_view() is None and g._lib.mdx_gsam_at_end(g._g) == 1, name


def test_tell_names_the_line_the_next_slab_starts_with(tmp_path, case):
    """301-byte blocks in slabs of 4 096 compressed bytes: the host parser started at the told pair yields exactly the
    records the device has not handed out yet — behind the second slab, behind the slab the long line starts in (its
    bytes are carried over several slabs: the pair stays blocks behind) and behind the last but one."""
    from mapdamage_amd.engine import DamageEngine
    ref, path, host = case
    text = path.read_bytes()
    gz = tmp_path / "x.sam.gz"
    u_of = dict(_write_blocks(gz, text, size=301)[::-1])         # compressed offset -> inflated offset of every block
    long_at = text.index(b"long1\t")
    tells, done = [], []
    with DamageEngine(LIBS, 70, 10, 0) as eng:
        eng.set_reference(ref)
        with sam.GpuSamStream(eng, str(gz), readgroups=list(LIB_OF.items()), chunk_bytes=4096, want_qual=True) as g:
            first = g.tell()
            n = 0
            while (v := g.next_view()) is not None:
                eng.sync()
                n += int(v.n_reads)
                tells.append(g.tell())
                done.append(n)
    assert n == host.batch.n and len(tells) > 20
    assert u_of[first[0]] + first[1] == text.index(b"\n", text.rindex(b"\n@")+ 1) + 1      # the first line behind the header
    at = [u_of[c] + p if c in u_of else None for c, p in tells]
    assert long_at in at
    k_long = at.index(long_at)
    # (the slab handed out next ends behind the long line: every slab in between lay within it)
    assert at[k_long + 1] > long_at + 40_000 and u_of[tells[k_long + 1][0]] - u_of[tells[k_long][0]] > 10 * 4096
    for k in (1, k_long, len(tells) - 2):
        with sam.compressed_text(str(gz), tells[k]) as handle:
            rest = sam.read_sam(handle, header=host.header)
        assert rest.batch.n == host.batch.n - done[k], k
        np.testing.assert_array_equal(rest.batch.pos, host.batch.pos[done[k]:])
        np.testing.assert_array_equal(rest.batch.seq_off, host.batch.seq_off[done[k]:] - host.batch.seq_off[done[k]])
        assert rest.qname == host.qname[done[k]:]


@pytest.mark.parametrize("golden,extra", GOLDENS)
def test_goldens_from_bgzipped_sam_on_the_device(tmp_path, golden, extra, monkeypatch):
    from mapdamage_amd.main import main
    g, path = _golden_sam(tmp_path, golden, extra)
    gz = tmp_path / "in.sam.gz"
    _bgzip(path, gz)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    want = [g.txt[f] for f in FILES]
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + extra
    runs = [tmp_path / "file", tmp_path / "pipe", tmp_path / "redirect"]
    assert main(["-i", str(gz), "-d", str(runs[0])] + [str(a) for a in base]) == 0
    assert _main_on_pipe(tmp_path, gz.read_bytes(), ["-d", runs[1]] + base, "devfd") == 0
    _, err, rc = _cli(["-i", "-", "-d", runs[2]] + base, stdin_file=gz, env={"MDX_GBAM_SLAB_BYTES": "65536"})
    assert rc == 0, err.decode()[-2000:]
    for out in runs:
        log = (out / "Runtime_log.txt").read_text()
        assert _tables(out) == want, out.name
        assert DEVICE in log and "bgzip-compressed SAM text, inflated and parsed on the device" in log, out.name


@pytest.mark.parametrize("golden,extra", GOLDENS)
def test_goldens_under_min_basequal_and_downsample(tmp_path, golden, extra, monkeypatch):
    """-Q 20 and --downsample 0.5 --downsample-seed 7 on the goldens' records: the bgzipped file on the device gives the
    tables of the plain-SAM run."""
    from mapdamage_amd.main import main
    _, path = _golden_sam(tmp_path, golden, extra)
    gz = tmp_path / "in.sam.gz"
    _bgzip(path, gz)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    for k, opts in enumerate((["-Q", "20"], ["--downsample", "0.5", "--downsample-seed", "7"])):
        base = [str(a) for a in ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + extra + opts]
        text, dev = tmp_path / ("text%d" % k), tmp_path / ("gz%d" % k)
        assert main(["-i", str(path), "-d", str(text)] + base) == 0
        assert main(["-i", str(gz), "-d", str(dev)] + base) == 0
        assert _tables(dev) == _tables(text), opts
        assert DEVICE in (dev / "Runtime_log.txt").read_text(), opts


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """20 000 records as SAM text, bgzipped (several slabs of 65 536 compressed bytes) and gzipped, with the FASTA."""
    tmp = tmp_path_factory.mktemp("many")
    ref = _genome()
    fasta.write_fasta(tmp / "ref.fa", ref)
    b, rg = _reads(ref, 20_000)
    path = tmp / "x.sam"
    _write_sam(path, ref, b, rg)
    _bgzip(path, tmp / "x.sam.gz")
    (tmp / "plain.sam.gz").write_bytes(gzip.compress(path.read_bytes(), 1))
    return tmp


@pytest.mark.parametrize("opts", [["-Q", "20"], ["--downsample", "0.5", "--downsample-seed", "7"]])
def test_many_slabs_equal_the_plain_text_run(tmp_path, many, opts, monkeypatch):
    from mapdamage_amd.main import main
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    base = ["-r", many / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + opts
    assert main(["-i", str(many / "x.sam"), "-d", str(tmp_path / "text")] + [str(a) for a in base]) == 0
    assert main(["-i", str(many / "x.sam.gz"), "-d", str(tmp_path / "file")] + [str(a) for a in base]) == 0
    assert _main_on_pipe(tmp_path, (many / "x.sam.gz").read_bytes(), ["-d", tmp_path / "pipe"] + base, "devfd") == 0
    for name in ("file", "pipe"):
        assert _tables(tmp_path / name) == _tables(tmp_path / "text"), name
        assert DEVICE in (tmp_path / name / "Runtime_log.txt").read_text()


def test_plain_gzip_and_two_ranks_take_the_host_path(tmp_path, many):
    from mapdamage_amd.main import main
    base = [str(a) for a in ("-r", many / "ref.fa", "--no-stats", "--log-level", "DEBUG")]
    assert main(["-i", str(many / "x.sam"), "-d", str(tmp_path / "text")] + base) == 0
    assert main(["-i", str(many / "plain.sam.gz"), "-d", str(tmp_path / "gzip")] + base) == 0
    log = (tmp_path / "gzip" / "Runtime_log.txt").read_text()
    assert _tables(tmp_path / "gzip") == _tables(tmp_path / "text")
    assert "plain gzip SAM text, read by the host (a gzip member has no blocks to share out" in log
    assert "Decode path: host decoder; fallbacks from the device path: 0" in log and "gave up" not in log
    # --gpus 2 (two ranks on one GPU, tables summed over gloo): SAM text, compressed or not, is the host's there
    _cli_ranks(["-i", many / "x.sam.gz", "-d", tmp_path / "ranks"] + base, gpus=2)
    assert _tables(tmp_path / "ranks") == _tables(tmp_path / "text")
    assert "Decode path: host decoder" in (tmp_path / "ranks" / "Runtime_log.txt").read_text()


def test_giving_up_and_damage(tmp_path):
    """A '\\r' line in a middle slab: from a pipe the host takes over at that slab (the log names the compressed offset and
    the records counted), from a file it reads the whole file again — the plain-text run's tables either way.  A flipped
    payload byte or CRC in a middle block goes through the inflater's and the CRC check's status: non-zero exit, an error
    in the log, no tables."""
    ref = _genome()
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    b, rg = _reads(ref, 1500)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg, extra=[_odd("carriage_return", 0)], at=1000)
    # (blocks of 20 000 bytes compress to a third: slabs of 65 536 compressed bytes hold about ten)
    gz = tmp_path / "x.sam.gz"
    _write_blocks(gz, path.read_bytes(), size=20_000)
    env = {"MDX_GBAM_SLAB_BYTES": "65536"}
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"]
    _, err, rc = _cli(["-i", path, "--host-decode", "-d", tmp_path / "text"] + base, data=b"", env=env)
    assert rc == 0, err.decode()[-2000:]
    for name, args, data in (("file", ["-i", gz], b""), ("pipe", ["-i", "-"], gz.read_bytes())):
        _, err, rc = _cli(args + ["-d", tmp_path / name] + base, data=data, env=env)
        assert rc == 0, err.decode()[-2000:]
        log = (tmp_path / name / "Runtime_log.txt").read_text()
        assert _tables(tmp_path / name) == _tables(tmp_path / "text"), name
        assert log.count("GPU decode path gave up") == 1 and "fallbacks from the device path: 1" in log, name
        if name == "pipe":
            line = [x for x in log.splitlines() if "gave up" in x][0]
            assert "from compressed offset" in line and "records are counted" in line and "offset 0 on" not in line
        else:
            assert "the whole file again" in log
    clean = tmp_path / "clean.sam"
    _write_sam(clean, ref, b, rg)
    starts = _write_blocks(tmp_path / "clean.sam.gz", clean.read_bytes(), size=20_000)
    raw = (tmp_path / "clean.sam.gz").read_bytes()
    mid = len(starts) // 2
    for name, where in (("payload", starts[mid][0] + 18 + 200), ("crc", starts[mid + 1][0] - 8)):
        bad = bytearray(raw)
        bad[where] ^= 0x10
        f = tmp_path / (name + ".sam.gz")
        f.write_bytes(bytes(bad))
        for how, args, data in (("file", ["-i", f], b""), ("pipe", ["-i", "-"], bytes(bad))):
            out = tmp_path / (name + "_" + how)
            _, err, rc = _cli(args + ["-d", out] + base, data=data, env=env)
            assert rc != 0, (name, how)
            log = (out / "Runtime_log.txt").read_text()
            assert "GPU decode path gave up: " in log and "the BGZF block at compressed offset %d" % starts[mid][0] in log, (name, how)
            assert "ERROR" in log and "compressed offset" in log.split("ERROR")[-1], (name, how)
            assert not any((out / t).exists() for t in FILES), (name, how)
