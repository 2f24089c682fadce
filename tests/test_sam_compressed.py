"""gzip- and bgzip-compressed SAM text on the host: `pysam.AlignmentFile(path)` (mapdamage/reader.py:38) lets htslib sniff
through compression, so `x.sam.gz` is SAM text whoever compressed it (stated from htslib's documentation; unpinned at the pysam
boundary).  The format is told by content, zlib inflates any number of members into ``read_sam``, the header is read without
reading further, and the host takes a file or a stream up at a (BGZF block, inflated bytes) pair.  Fixtures come from the
project's own BGZF writer and from blocks made by hand (tests/test_fasta_bgzf.py)."""
import gzip
import os

import numpy as np
import pytest

from mapdamage_amd import sam, synth
from tests.test_fasta_bgzf import _bgzip, _block, _write_blocks
from tests.test_pipe_input import _Pipe, _write

RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s2", "LB": "lib2"}]
COLUMNS = ("flag", "tid", "pos", "tlen", "cigar", "seq", "qual", "seq_off", "cigar_off")


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    """SAM text of 700 records in two read groups whose last line has no newline, and what ``read_sam`` makes of it."""
    tmp = tmp_path_factory.mktemp("samtext")
    ref = synth.make_genome(seed=3, sizes=(("chr1", 50_000), ("chr2", 9_000)), n_run=10, lower_run=100)
    b = synth.make_reads(ref, 700, 9, len_range=(30, 120), with_qual=True, frac_softclip=0.1, frac_ins=0.05, frac_del=0.05)
    path = tmp / "x.sam"
    sam.write_sam(str(path), b, ref.names, ref.lengths, RGS, [RGS[i % 2]["ID"] for i in range(b.n)])
    data = path.read_bytes().rstrip(b"\n")
    path.write_bytes(data)
    return data, sam.read_sam(str(path))


def _forms(tmp_path, data):
    """name -> (path, format) of the same text: plain, bgzipped in 0xFF00- and 301-byte blocks, gzipped in one member and two."""
    out = {}
    p = tmp_path / "plain.sam"
    p.write_bytes(data)
    out["plain"] = (p, sam.SAM_TEXT)
    (tmp_path / "raw").write_bytes(data)
    p = tmp_path / "big.sam.gz"
    _bgzip(tmp_path / "raw", p)
    out["bgzf 0xFF00"] = (p, sam.SAM_BGZF)
    p = tmp_path / "small.sam.gz"
    _write_blocks(p, data, size=301)
    out["bgzf 301"] = (p, sam.SAM_BGZF)
    p = tmp_path / "one.sam.gz"
    p.write_bytes(gzip.compress(data))
    out["gzip"] = (p, sam.SAM_GZIP)
    p = tmp_path / "two.sam.gz"
    cut = len(data) // 3
    p.write_bytes(gzip.compress(data[:cut]) + gzip.compress(data[cut:]))
    out["two members"] = (p, sam.SAM_GZIP)
    return out


def _same(got, want):
    assert got.header.text == want.header.text
    for k in COLUMNS:
        np.testing.assert_array_equal(getattr(got.batch, k), getattr(want.batch, k), err_msg=k)
    assert list(got.rg) == list(want.rg) and got.qname == want.qname


def test_the_four_formats_are_told_apart(tmp_path, text):
    data, _ = text
    forms = _forms(tmp_path, data)
    bam = _write(tmp_path, n=300)
    forms["bam"] = (bam, sam.BAM)
    # behind an empty first member: BGZF stays BGZF (the member carries BC), plain gzip stays plain gzip, BAM stays BAM
    p = tmp_path / "empty_first_bgzf.sam.gz"
    p.write_bytes(_block(b"") + forms["bgzf 301"][0].read_bytes())
    forms["empty first, bgzf"] = (p, sam.SAM_BGZF)
    p = tmp_path / "empty_first_gzip.sam.gz"
    p.write_bytes(gzip.compress(b"") + forms["gzip"][0].read_bytes())
    forms["empty first, gzip"] = (p, sam.SAM_GZIP)
    p = tmp_path / "empty_first.bam"
    p.write_bytes(_block(b"") + bam.read_bytes())
    forms["empty first, bam"] = (p, sam.BAM)
    for seed, (name, (path, want)) in enumerate(forms.items()):
        assert sam.input_format(str(path)) == want, name
        assert sam.is_bam(str(path)) == (want == sam.BAM), name
        pipe = _Pipe(tmp_path, path.read_bytes(), "pipe", seed)
        with pipe.source() as src:
            assert sam.input_format(src) == want, name
            assert sam.input_format(src) == want, name      # (a second sniff sees the same bytes)
            assert sam.is_bam(src) == (want == sam.BAM), name
        pipe.finish()
    # what inflates to nothing is SAM text too — nothing but an end-of-file block, an empty gzip member —: no records
    for name, data, want in (("eof.sam.gz", _block(b""), sam.SAM_BGZF), ("empty.sam.gz", gzip.compress(b""), sam.SAM_GZIP)):
        p = tmp_path / name
        p.write_bytes(data)
        assert sam.input_format(str(p)) == want and not sam.is_bam(str(p)), name
        assert sam.read_alignments(str(p)).batch.n == 0 and sam.sam_header(str(p))[1] == 0, name
    # ... and bytes behind 1f 8b that do not inflate at all are the BAM decoders' to word
    p = tmp_path / "junk.gz"
    p.write_bytes(b"\x1f\x8b\x08\x00" + b"\xff" * 64)
    assert sam.input_format(str(p)) == sam.BAM
    # two bytes tell uncompressed text: the sniff of a stream waits for no more
    r, w = os.pipe()
    os.write(w, b"@HD")
    with sam.Source("/dev/fd/%d" % r) as src:
        os.close(r)
        assert sam.input_format(src) == sam.SAM_TEXT
    os.close(w)
    # a stream's path is still never opened for the sniff
    r, w = os.pipe()
    try:
        with pytest.raises(ValueError, match="stream"):
            sam.input_format("/dev/fd/%d" % r)
        with pytest.raises(ValueError, match="stream"):
            sam.is_bam("/dev/fd/%d" % r)
    finally:
        os.close(r)
        os.close(w)


def test_read_alignments_reads_every_form(tmp_path, text):
    data, want = text
    for seed, (name, (path, _)) in enumerate(_forms(tmp_path, data).items()):
        _same(sam.read_alignments(str(path)), want)
        pipe = _Pipe(tmp_path, path.read_bytes(), "pipe", seed)
        with pipe.source() as src:
            _same(sam.read_alignments(src), want)
        pipe.finish()


def test_sam_header_of_compressed_text(tmp_path, text):
    from mapdamage_amd.reader import BAMReader
    data, want = text
    lines = data.split(b"\n")
    body = sum(len(x) + 1 for x in lines if x.startswith(b"@"))
    for seed, (name, (path, _)) in enumerate(_forms(tmp_path, data).items()):
        header, off = sam.sam_header(str(path))
        assert header.text == want.header.text and off == body, name
        pipe = _Pipe(tmp_path, path.read_bytes(), "pipe", seed)
        with pipe.source() as src:
            header, off = sam.sam_header(src)
            assert header.text == want.header.text and off == body, name
            _same(sam.read_alignments(src), want)              # (nothing was consumed)
        pipe.finish()
        reader = BAMReader(str(path), sam_header_only=True)
        assert reader.handle.header.text == want.header.text and reader.handle.batch.n == 0 and not reader.is_bam
        batches = list(reader.iter_batches())
        assert sum(b.n for b in batches) == int(((want.batch.flag & 0xF04) == 0).sum())
        reader.close()
    # header only, compressed: the whole text is the header
    head = data[:body]
    p = tmp_path / "head.sam.gz"
    _write_blocks(p, head, size=97)
    header, off = sam.sam_header(str(p))
    assert header.text == want.header.text and off == len(head)


@pytest.mark.parametrize("stream", [False, True])
def test_the_host_resumes_at_a_block_and_phase(tmp_path, text, stream):
    """(compressed offset of a BGZF block, inflated bytes to drop) in the middle of a run of lines — the pair names a line's
    first byte, blocks in front of where the line starts or the very block —: exactly the records behind it."""
    from mapdamage_amd.reader import BAMReader
    data, want = text
    path = tmp_path / "x.sam.gz"
    starts = _write_blocks(path, data, size=301)
    kept = (want.batch.flag & 0xF04) == 0
    lines = data.split(b"\n")
    n_head = sum(1 for x in lines if x.startswith(b"@"))
    for k, back in ((n_head + 250, 0), (n_head + 411, 3)):
        at = sum(len(x) + 1 for x in lines[:k])             # the line's first byte in the text
        b = max(i for i, (_, u) in enumerate(starts) if u <= at) - back
        resume = (starts[b][0], at - starts[b][1])
        pipe = _Pipe(tmp_path, path.read_bytes(), "pipe", k) if stream else None
        reader = BAMReader(pipe.path if stream else str(path), sam_header_only=True, source=pipe.source() if stream else None)
        got = list(reader.iter_batches(resume=resume))
        reader.close()
        if pipe is not None:
            pipe.finish()
        first = k - n_head
        assert sum(x.n for x in got) == int(kept[first:].sum())
        np.testing.assert_array_equal(np.concatenate([x.pos for x in got]), want.batch.pos[first:][kept[first:]])
        np.testing.assert_array_equal(np.concatenate([x.flag for x in got]), want.batch.flag[first:][kept[first:]])


def test_damage_is_worded_by_the_host(tmp_path, text):
    data, _ = text
    pieces = [data[lo:lo + 3000] for lo in range(0, len(data), 3000)]
    bad_crc = b"".join(_block(p, crc=1 if i == 2 else None) for i, p in enumerate(pieces)) + _block(b"")
    p = tmp_path / "crc.sam.gz"
    p.write_bytes(bad_crc)
    with pytest.raises(sam.BAMError, match="compressed offset"):
        sam.read_alignments(str(p))
    whole = b"".join(_block(x) for x in pieces)
    p = tmp_path / "cut.sam.gz"
    p.write_bytes(whole[:len(whole) - 11])
    with pytest.raises(sam.BAMError, match="cut short"):
        sam.read_alignments(str(p))
