"""BAM and SAM from stdin, pipes and named pipes through the input source of libmdx.so (include/mdx.h mdx_source_*): the
host decoders read a stream exactly as they read the same bytes from a file, the format is sniffed without losing a byte,
damage gives the file's error, and memory stays bounded however long the stream is.  Host code only: no GPU."""
import json
import os
import pathlib
import subprocess
import sys
import threading

import numpy as np
import pytest

from mapdamage_amd import sam, synth

ROOT = pathlib.Path(__file__).resolve().parent.parent
RGS = [{"ID": "rgA", "SM": "s", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s", "LB": "lib2"}, {"ID": "x", "SM": "s", "LB": "lib1"}]
# the BGZF layouts of tests/test_gpu_decode.py: htslib's, one stream cut every 0xFF00 bytes, htsjdk's 65 498, tiny blocks
LAYOUTS = {"htslib": dict(), "cut": dict(htslib_blocks=False), "htsjdk": dict(htslib_blocks=False, block_bytes=65498),
           "tiny": dict(htslib_blocks=False, block_bytes=90)}
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from mapdamage_amd import build
    build.build_lib()


def _write(tmp_path, n=6000, seed=4, layout="htslib"):
    ref = synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)
    b = synth.make_reads(ref, n, seed, len_range=(25, 160), paired=True, frac_softclip=0.2, frac_ins=0.08, frac_del=0.08,
                         frac_skip=0.01, with_qual=True, frac_filtered=0.05)
    rng = np.random.default_rng(seed)
    rg = [RGS[i]["ID"] for i in rng.integers(0, 3, size=b.n)]
    path = tmp_path / ("%s.bam" % layout)
    sam.write_bam(str(path), b, ref.names, ref.lengths, RGS, rg_of_record=rg, **LAYOUTS[layout])
    return path


def _feed(fd, data, seed=0):
    """Writes ``data`` to ``fd`` in irregular pieces (1 B ... 1 MiB) and closes it; a reader that leaves early is no error."""
    rng = np.random.default_rng(seed)
    sizes = [1, 7, 100, 4096, 65535, 65536, 300_001, 1 << 20]
    try:
        at = 0
        while at < len(data):
            k = int(sizes[int(rng.integers(0, len(sizes)))])
            at += os.write(fd, data[at:at + k])
    except (BrokenPipeError, OSError):
        pass
    finally:
        os.close(fd)


class _Pipe:
    """An os.pipe() (read as /dev/fd/N) or a named pipe, fed by a writer thread."""

    def __init__(self, tmp_path, data, kind="pipe", seed=0):
        self.kind = kind
        if kind == "pipe":
            r, w = os.pipe()
            self.path, self._r = "/dev/fd/%d" % r, r
            self.thread = threading.Thread(target=_feed, args=(w, data, seed), daemon=True)
        else:
            self.path, self._r = str(tmp_path / ("fifo%d" % seed)), None
            os.mkfifo(self.path)
            self.thread = threading.Thread(target=lambda: _feed(os.open(self.path, os.O_WRONLY), data, seed), daemon=True)
        self.thread.start()

    def source(self):
        src = sam.Source(self.path)
        if self._r is not None:
            os.close(self._r)        # (the source holds a descriptor of its own)
            self._r = None
        assert src.is_stream
        return src

    def finish(self):
        if self._r is not None:
            os.close(self._r)
        self.thread.join(timeout=60)
        assert not self.thread.is_alive()


def _columns(al):
    b = al.batch
    names = [al.rg_names[i] if i >= 0 else None for i in al.rg_index.tolist()]
    return dict(flag=b.flag, tid=b.tid, pos=b.pos, tlen=b.tlen, cigar=b.cigar, ncig=np.diff(b.cigar_off.astype(np.int64)),
                seq=b.seq, qual=b.qual, nseq=np.diff(b.seq_off.astype(np.int64)), rg=np.asarray(names, dtype=object),
                qmin=al.qmin)


def _concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0) for k in (parts[0] if parts else {})}


def _chunked(src, chunk_bytes):
    with sam.BamStream(src, chunk_bytes=chunk_bytes) as st:
        header = st.header
        parts = [_columns(c) for c in st]
    return header, _concat(parts)


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _cases(tmp_path):
    for layout in LAYOUTS:
        yield layout, _write(tmp_path, n=1500 if layout == "tiny" else 6000, layout=layout)
    for name in ("foreign.bam", "foreign_nocg.bam", "foreign_nolb.bam"):
        yield name, GOLDEN / name


@pytest.mark.parametrize("kind", ["pipe", "fifo"])
def test_host_decoders_read_a_pipe_as_they_read_the_file(tmp_path, kind):
    """Both host decoders over a pipe: the columns, header and read groups of the same bytes decoded from the file."""
    seed = 0
    for name, path in _cases(tmp_path):
        whole = sam.read_bam_native(str(path))
        want = _columns(whole)
        for chunk in (1 << 16, 1 << 20, 256 << 20):
            seed += 1
            p = _Pipe(tmp_path, path.read_bytes(), kind, seed)
            with p.source() as src:
                header, got = _chunked(src, chunk)
            p.finish()
            assert header.references == whole.header.references and header.lengths == whole.header.lengths, name
            assert header.text == whole.header.text
            _equal(got, want)
        seed += 1
        p = _Pipe(tmp_path, path.read_bytes(), kind, seed)
        with p.source() as src:
            one = sam.read_bam_native(src)
        p.finish()
        # (the read-group table is in the order the decoding threads met the names: the records' names are compared)
        assert one.header.text == whole.header.text and set(one.rg_names) == set(whole.rg_names), name
        _equal(_columns(one), want)


def test_sniffing_through_the_source_loses_no_byte(tmp_path):
    """BAM or SAM text by the first bytes of the stream, which are still there for the decode: a SAM file through a pipe
    gives the records ``read_sam`` finds in the file."""
    ref = synth.make_genome(seed=3, sizes=(("chr1", 50_000),), n_run=10, lower_run=100)
    b = synth.make_reads(ref, 800, 9, len_range=(30, 90), with_qual=True, frac_softclip=0.1)
    samp = tmp_path / "x.sam"
    sam.write_sam(str(samp), b, ref.names, ref.lengths, RGS[:1], ["rgA"] * b.n)
    bam = _write(tmp_path, n=500)
    for path, is_bam in ((samp, False), (bam, True)):
        p = _Pipe(tmp_path, path.read_bytes(), "pipe", 5)
        with p.source() as src:
            assert sam.is_bam(src) == is_bam
            assert sam.is_bam(src) == is_bam          # (a peek leaves the bytes where they are)
            got = sam.read_alignments(src)
        p.finish()
        want = sam.read_alignments(str(path))
        assert got.header.text == want.header.text
        if is_bam:
            _equal(_columns(got), _columns(want))
        else:
            for k in ("flag", "tid", "pos", "tlen", "cigar", "seq", "qual", "seq_off", "cigar_off"):
                np.testing.assert_array_equal(getattr(got.batch, k), getattr(want.batch, k), err_msg=k)
            assert list(got.rg) == list(want.rg) and got.qname == want.qname
    # a stream's path is never opened for the sniff (its bytes would be lost to the run)
    r, w = os.pipe()
    try:
        with pytest.raises(ValueError, match="stream"):
            sam.is_bam("/dev/fd/%d" % r)
    finally:
        os.close(r)
        os.close(w)


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from mapdamage_amd.reader import BAMReader
down = None if sys.argv[2] == "none" else float(sys.argv[2])
down = int(down) if down is not None and down >= 1 else down
r = BAMReader("-", downsample_to=down, downsample_seed=7, chunk_bytes=int(sys.argv[3]))
out = {"refs": sorted(r.get_references().items()), "libs": r.get_libraries(), "stream": r.is_stream,
       "flag": [], "pos": [], "lib": []}
for b in r.iter_batches():
    out["flag"] += b.flag.tolist(); out["pos"] += b.pos.tolist(); out["lib"] += b.lib.tolist()
r.close()
print(json.dumps(out))
"""


def _reader_over_stdin(data, down, chunk_bytes):
    out, err, rc = _child([sys.executable, "-c", _CHILD, str(ROOT), str(down), str(chunk_bytes)], data, timeout=300)
    assert rc == 0, err.decode()
    return json.loads(out)


def _child(cmd, data, timeout, seed=3, env=None, cwd=None):
    """``cmd`` with ``data`` on its stdin — a true pipe, fed by a writer thread — under a time limit: stdout, stderr, exit."""
    r, w = os.pipe()
    try:
        proc = subprocess.Popen(cmd, stdin=r, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=cwd)
    finally:
        os.close(r)
    t = threading.Thread(target=_feed, args=(w, data, seed), daemon=True)
    t.start()
    try:
        out, err = proc.communicate(timeout=timeout)
    finally:
        if proc.poll() is None:
            proc.kill()
            proc.wait()
        t.join(timeout=60)
    assert not t.is_alive()
    return out, err, proc.returncode


@pytest.mark.parametrize("down,chunk_bytes", [("none", 1 << 20), ("none", 0), (0.3, 1 << 18), (500, 1 << 20)])
def test_bamreader_reads_bam_from_stdin(tmp_path, down, chunk_bytes):
    """``BAMReader("-")`` with BAM on stdin (a true pipe): the references, libraries and records of the file; the
    fraction and the fixed-number downsampling follow the Python RNG as they do for the file."""
    from mapdamage_amd.reader import BAMReader
    path = _write(tmp_path, n=5000, layout="cut")
    got = _reader_over_stdin(path.read_bytes(), down, chunk_bytes)
    d = None if down == "none" else down
    r = BAMReader(str(path), downsample_to=d, downsample_seed=7, chunk_bytes=chunk_bytes or None)
    want = {"flag": [], "pos": [], "lib": []}
    for b in r.iter_batches():
        want["flag"] += b.flag.tolist(); want["pos"] += b.pos.tolist(); want["lib"] += b.lib.tolist()
    assert got["stream"] is True
    assert got["refs"] == [list(x) for x in sorted(r.get_references().items())]
    assert got["libs"] == [list(x) for x in r.get_libraries()]
    for k in want:
        assert got[k] == want[k], k
    assert len(got["pos"]) > 0


def _message(exc):
    """An error's text without the input's name in front."""
    text = str(exc)
    return text.split("': ", 1)[1] if "': " in text else text


def test_damage_gives_the_files_error(tmp_path):
    """A stream that ends inside a block, a damaged block, an empty stream: the error of the same bytes in a file, from
    both host decoders, within the time limit — the writer is never left blocked."""
    raw = _write(tmp_path, n=4000, layout="cut").read_bytes()
    bad = bytearray(raw)
    bad[len(raw) // 2] ^= 0x55
    cases = {"truncated": raw[:len(raw) // 2 + 7], "damaged": bytes(bad), "empty": b"", "header only": raw[:40]}
    seed = 100
    for name, data in cases.items():
        f = tmp_path / ("case_%d.bam" % seed)
        f.write_bytes(data)
        for decode in ("one-piece", "chunked"):
            def run(src):
                if decode == "one-piece":
                    return sam.read_bam_native(src)
                return _chunked(src, 1 << 16)
            with pytest.raises(ValueError) as want:
                run(str(f))
            seed += 1
            p = _Pipe(tmp_path, data, "pipe", seed)
            with p.source() as src:
                with pytest.raises(ValueError) as got:
                    run(src)
            p.finish()
            assert _message(got.value) == _message(want.value), (name, decode)


def test_a_seek_behind_the_window_is_an_error_not_a_hang(tmp_path):
    """What a stream's consumer has let go of is gone: going back there is a clear error."""
    path = _write(tmp_path, n=30_000, layout="htslib")
    p = _Pipe(tmp_path, path.read_bytes(), "pipe", 9)
    with p.source() as src:
        with sam.BamStream(src, chunk_bytes=1 << 20) as st:
            n = 0
            for c in st:
                n += c.batch.n
            assert n == 30_000
            with pytest.raises(ValueError, match="behind the part of the stream still held"):
                st.seek(0, 0)
    p.finish()


def _blocks(data):
    """(offset, size, ISIZE) of every BGZF block of ``data``."""
    out, off = [], 0
    while off < len(data):
        xlen = int.from_bytes(data[off + 10:off + 12], "little")
        bsize = int.from_bytes(data[off + 16:off + 18], "little") + 1
        out.append((off, bsize, int.from_bytes(data[off + bsize - 4:off + bsize], "little")))
        off += bsize
        assert xlen == 6
    return out


_RSS_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from mapdamage_amd import sam
src = sam.Source("-")
n = 0
with sam.BamStream(src, chunk_bytes=1 << 20) as st:
    for c in st:
        n += c.batch.n
src.close()
# (the peak RSS of this process image: VmHWM starts afresh at exec — ru_maxrss would carry over the forking parent's)
hwm = [int(line.split()[1]) for line in open("/proc/self/status") if line.startswith("VmHWM:")][0]
print(n, hwm * 1024)
"""


def test_memory_stays_bounded_however_long_the_stream(tmp_path):
    """An htslib-layout file's record blocks repeated k times behind its header (which sits in blocks of its own), ended
    by the EOF block, decoded from stdin in 1 MiB chunks: a stream four times as long raises the child's peak RSS by less
    than the shorter stream's compressed size (a source that held what it has read would grow by three times that)."""
    import zlib
    path = _write(tmp_path, n=30_000, layout="htslib")
    data = path.read_bytes()
    blocks = _blocks(data)
    assert blocks[-1][2] == 0                           # the EOF block
    # the inflated header: magic, l_text, text, n_ref, then the reference dictionary
    head = b"".join(zlib.decompress(data[o:o + s], 31) for o, s, _ in blocks[:4])
    l_text = int.from_bytes(head[4:8], "little")
    n_ref = int.from_bytes(head[8 + l_text:12 + l_text], "little")
    off = 12 + l_text
    for _ in range(n_ref):
        off += 8 + int.from_bytes(head[off:off + 4], "little")
    header_bytes, acc = None, 0
    for o, s, isize in blocks:
        acc += isize
        if acc >= off:
            assert acc == off, "the header shares a block with records"
            header_bytes = o + s
            break
    records = data[header_bytes:blocks[-1][0]]
    eof = data[blocks[-1][0]:]

    def run(reps):
        stream = data[:header_bytes] + records * reps + eof
        out, err, rc = _child([sys.executable, "-c", _RSS_CHILD, str(ROOT)], stream, timeout=600, seed=11)
        assert rc == 0, err.decode()
        n, rss = map(int, out.split())
        assert n == 30_000 * reps
        return len(stream), rss

    size_short, rss_short = run(4)
    size_long, rss_long = run(16)
    assert size_long > 3.9 * size_short
    assert rss_long - rss_short < size_short, (rss_short, rss_long, size_short)
